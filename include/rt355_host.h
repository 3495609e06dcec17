/* rt355_host.h — C-ABI of the host-side producers (librt355_host.so): the Scene primitive /
 * material factory, the BVH2 / SBVH / BVH4 / TLAS builders, the camera maths and a Renderer
 * mirror.  These wrap the C++ classes of magr_ray_tracer_amd/host/rt_host.h, which mirror the
 * reference's Scene (src/scene.h:5-34), BVH2/BVH4 (src/bvh.h:4-56), TLAS (src/tlas.h:2-12),
 * CameraManager (src/camera.h:7-122) and Renderer (src/renderer.h:44-120).
 * All functions return 0 on success, negative on failure (rth_last_error() has the text).
 */
#ifndef RT355_HOST_H
#define RT355_HOST_H
#include "rt355_types.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct RthScene RthScene;
typedef struct RthRenderer RthRenderer;

const char* rth_last_error(void);

/* Scene::Scene / ~Scene (scene.cpp:8-10,74) */
RthScene* rth_scene_create(void);
void      rth_scene_destroy(RthScene* s);
/* Scene::AddMaterial (scene.cpp:84-100): pushes a zeroed material (texIdx -1), then copies the
 * fields of *init if given; returns the material index. */
int rth_add_material(RthScene* s, const char* name, const RtMaterial* init);
/* Scene::LoadTexture minus the file read (scene.cpp:244-256): appends texels, adds a material. */
int rth_add_texture(RthScene* s, const char* name, const RtFloat4* texels, int width, int height);
/* Scene::LoadTexture (scene.cpp:244-256) for PNG, JPEG, TGA and Radiance HDR files, texel rule of stbi_loadf; returns the material index or -1. */
int rth_load_texture(RthScene* s, const char* filename, const char* name);
int rth_add_sphere(RthScene* s, const float pos[3], float radius, const char* material);       /* scene.cpp:125-138 */
int rth_add_plane(RthScene* s, const float N[3], float d, const char* material);               /* scene.cpp:140-150 */
int rth_add_triangle(RthScene* s, const float v0[3], const float v1[3], const float v2[3],
                     const float uv0[2], const float uv1[2], const float uv2[2], const char* material, int flipNormal); /* scene.cpp:158-176 */
int rth_add_quad(RthScene* s, const float v0[3], const float v1[3], const float v2[3], const float v3[3],
                 const char* material, int flipNormal);                                       /* scene.cpp:152-156, default uvs */
/* n x AddTriangle; verts is n*9 floats (v0,v1,v2), uvs n*6 floats or NULL (all zero). */
int rth_add_triangles(RthScene* s, const float* verts, const float* uvs, int n, const char* material, int flipNormal);
/* Scene::LoadModel (scene.cpp:178-243): OBJ (+MTL map_Kd names); returns the number of triangles added or -1. */
int rth_load_model(RthScene* s, const char* filename, const char* defaultMaterial, const float pos[3], int forceDefaultMat);
/* SaveImageF (template/template.cpp:1629-1644): float4 image -> 8-bit RGB PNG, bytes (uchar)(min(c,1)*255). */
int rth_save_png(const char* file, int width, int height, const RtFloat4* data);
/* BVH2::BuildBLAS(true, startIdx) with bvh2->alpha = alpha (bvh.cpp:46-82). */
int rth_build_blas(RthScene* s, int startIdx, float alpha);
/* Threads for the following BuildBLAS calls: 1 = the reference's sequential loop; > 1 = task-parallel subtrees numbered
 * afterwards in the reference's LIFO order (identical arrays). */
int rth_set_build_threads(RthScene* s, int threads);
/* The linear BVH builder (rt_build_bvh2, rt355.h) over primitives [startIdx, end), appended as BuildBLAS appends a BLAS: instance
 * record, node and primIdx arrays, rth_bvh_stats; rth_build_bvh4 / rth_build_tlas / rth_renderer_* take it unchanged.  device >= 0:
 * on that GPU; -1: the host restatement (identical arrays).  opts NULL = defaults.  Returns RT_E_* and leaves the scene unchanged
 * when the build is refused. */
int rth_build_blas_lbvh(RthScene* s, int startIdx, int device, const RtBuildOptions* opts);
int rth_lbvh_stats(RthScene* s, RtBuildStats* out);   /* statistics of the scene's last rth_build_blas_lbvh */
/* The host restatement on caller arrays: rt_build_bvh2's contract without the device (stats->device_ms = 0). */
int rth_build_bvh2_lbvh(const RtBuildOptions* opts, const RtPrimitive* prims, int32_t nPrims, int32_t first, int32_t count,
                        uint32_t nodeBase, uint32_t idxBase, RtBVHNode2* nodes, int32_t nodeCap, int32_t* nNodes, uint32_t* primIdx,
                        RtBuildStats* stats);
/* The GPU build of the default SAH BLAS (rt_build_bvh2_sah, rt355.h) over primitives [startIdx, end), appended exactly as
 * rth_build_blas(s, startIdx, 1) appends it (instance record, nodes, primIdx, rth_bvh_stats); mixes BLAS by BLAS with the other
 * builders.  device >= 0: on that GPU; -1: the host restatement.  Returns RT_E_* and leaves the scene unchanged when refused. */
int rth_build_blas_sah_gpu(RthScene* s, int startIdx, int device);
/* The host restatement on caller arrays: rt_build_bvh2_sah's contract without the device (stats->device_ms = 0). */
int rth_build_bvh2_sah(const RtPrimitive* prims, int32_t nPrims, int32_t first, int32_t count, uint32_t nodeBase, uint32_t idxBase,
                       RtBVHNode2* nodes, int32_t nodeCap, int32_t* nNodes, uint32_t* primIdx, RtBuildStats* stats);
/* SBVH trees by the GPU builder (rt_build_bvh2_sbvh, rt355.h) over primitives [startIdx, end), appended exactly as
 * rth_build_blas(s, startIdx, alpha) appends them (instance record, nodes, primIdx, rth_bvh_stats including spatial splits and clipped
 * primitives).  device >= 0: on that GPU; -1: the host restatement.  Returns RT_E_* and leaves the scene unchanged when refused. */
int rth_build_blas_sbvh_gpu(RthScene* s, int startIdx, float alpha, int device);
/* The host restatement on caller arrays: rt_build_bvh2_sbvh's contract without the device (stats->device_ms = 0). */
int rth_build_bvh2_sbvh(float alpha, const RtPrimitive* prims, int32_t nPrims, int32_t first, int32_t count, uint32_t nodeBase,
                        uint32_t idxBase, RtBVHNode2* nodes, int32_t nodeCap, int32_t* nNodes, uint32_t* primIdx, int32_t idxCap,
                        int32_t* nIdx, RtSbvhStats* stats);
/* The host restatement of rt_update_scene (rt355.h): rth_set_primitives replaces primitives [first, first + count), which must keep
 * their objType and matIdx; rth_refit refits every BLAS of the scene's BVH2 in place by the rules rt_update_scene runs on the device
 * (csrc/refit_common.h).  The caller then runs rth_build_tlas (and rth_build_bvh4 if it renders a BVH4).  Both return RT_E_* and
 * change nothing when refused. */
int rth_set_primitives(RthScene* s, int first, int count, const RtPrimitive* prims);
int rth_refit(RthScene* s);
/* The host restatement of RtGeometry's vertex form (rt355.h): triangles [first, first + count) move to the vertices at positions
 * (vertex j at positions + j * strideBytes; nVertices of them) named by indices (3 * count of them; NULL: 3i, 3i + 1, 3i + 2), by the
 * rule of csrc/geometry_common.h that k_tri_from_vertices compiles too: v0, v1, v2, N, centroid and area anew, everything else of the
 * record as it is.  The refusals are the device call's (a non-triangle in the window, a bad stride, too few vertices, an index >=
 * nVertices, ...): RT_E_INVALID, and nothing has changed.  rth_refit next, as after rth_set_primitives. */
int rth_set_vertices(RthScene* s, int first, int count, const float* positions, int64_t strideBytes, int64_t nVertices, const uint32_t* indices);
/* The host restatement of rt_rebuild_scene's BLAS rebuild (rt355.h): discards the scene's BVH2 and builds every distinct BLAS again
 * over the primitive range it covers (in increasing order of the ranges, appended as BuildBLAS appends BLAS after BLAS) with the host
 * restatement of the chosen builder: RT_REBUILD_SAH (rth_build_bvh2_sah; opts ignored), RT_REBUILD_LBVH (rth_build_bvh2_lbvh, opts
 * NULL = defaults) or RT_REBUILD_SBVH (rth_build_bvh2_sbvh with opts->alpha, NULL or zero-filled = 0; alpha outside [0, 1] is
 * RT_E_INVALID; every BLAS appends the nodes and indices its tree turned out to have, and the scene's spatial-split, clipped-primitive
 * and forced-leaf statistics become the sums).  Instance transforms stay, every bvhIdx becomes its BLAS's new root.  The caller then runs rth_build_tlas (and
 * rth_build_bvh4).  Returns RT_E_* and changes nothing when refused (a scene whose BLAS do not cover contiguous, disjoint, ordered
 * ranges; whatever the builder refuses). */
int rth_rebuild(RthScene* s, int builder, const RtBuildOptions* opts);
/* The host restatement of rt_rebuild_ranges (rt355.h): rth_rebuild under a plan, plan[nRanges] with one RT_REBUILD_SAH / LBVH / SBVH /
 * KEEP / REFIT_RANGE per distinct BLAS in increasing order of the ranges.  A built BLAS is appended as rth_rebuild appends it; a kept one as
 * its bound block of nodes, relocated by the rule the device applies (csrc/rebuild_common.h, relocated_first), with its primIdx slots
 * unchanged; a refit one likewise, then its boxes are made anew from the scene's primitives by rth_refit's rules over that block alone.
 * Refused like rth_rebuild, and by rt_rebuild_ranges' plan rules: RT_E_INVALID for a null plan, a wrong nRanges, an unknown word or
 * RT_REBUILD_REFIT; RT_E_UNSUPPORTED for RT_REBUILD_KEEP or RT_REBUILD_REFIT_RANGE of a BLAS that is not compact.  (The primitives a kept BLAS covers must not
 * have changed since it was built or refit: the host scene has no window to check that against.) */
int rth_rebuild_ranges(RthScene* s, const int32_t* plan, int nRanges, const RtBuildOptions* opts);
/* rt_blas_ranges (rt355.h) of the scene's arrays: the primitive range of every instance's BLAS; RT_E_UNSUPPORTED (rt_last_error() has
 * the reason) when the scene is not of the shape a rebuild takes. */
int rth_blas_ranges(RthScene* s, int32_t* firstOut, int32_t* countOut);
int rth_build_bvh4(RthScene* s);            /* new BVH4(*bvh2) (scene.cpp:71)                    */
/* new TLAS(*bvh2); Build() (renderer.cpp:12-13).  Refused (-1, the scene keeps the TLAS it had) for more than 256 instances, none, a
 * singular transform, and where the clustering finds no partner: no two boxes with a union area below RT_REALLYFAR (instances 1e15
 * apart, NaN boxes), which rt_update_scene / rt_rebuild_scene refuse as RT_E_UNSUPPORTED and the reference answers by reading slot[-1]. */
int rth_build_tlas(RthScene* s);
/* BVH4::Convert + Collapse (bvh.cpp:695-787) on a caller-provided BVH2 node array, one BLAS rooted at node 0; out[n] */
int rth_bvh4_from_nodes(const RtBVHNode2* nodes, int n, RtBVHNode4* out);
/* rth_build_bvh4's arrays by the level-wise collapse (rt_build_bvh4, rt355.h): device >= 0: on that GPU; -1: the host restatement.
 * Returns RT_E_* and leaves the scene's BVH4 as it was when refused. */
int rth_build_bvh4_gpu(RthScene* s, int device);
/* The host restatement of rt_build_bvh4 (rt355.h): the same level loop over csrc/collapse_common.h, written sequentially, with the
 * same checks and messages (in rth_last_error()); stats->device_ms = 0.  Optional outputs (NULL: not wanted) of what the upload
 * derives from the collapsed tree: quads (8 RtFloat4 per live node, room for nNodes records), rootEntry[nRoots] (the live id of every
 * root), quadNode (live id -> node id, room for nNodes). */
int rth_build_bvh4_levels(const RtBVHNode2* nodes2, int32_t nNodes, int32_t nIdx, const uint32_t* roots, int32_t nRoots, RtBVHNode4* out4,
                          RtBvh4Stats* stats, RtFloat4* quads, uint32_t* rootEntry, uint32_t* quadNode);
/* The host restatement of RT_REBUILD_REFIT's collapse (rt355.h), sequential over csrc/collapse_common.h.  refit2: the BVH2 after the
 * refit (same topology as before it); inout4: the collapse of the BVH2 before the refit; quadNode[nLive]: its live nodes by live id
 * (rth_build_bvh4_levels' quadNode).  Writes Convert's record of every node plus the recomputed records of the live nodes and counts
 * in *changedNodes (may be NULL) the live records that differ from inout4's in a slot's (first, count); when that count is not zero it
 * collapses level by level instead.  Either way inout4 ends up as rth_build_bvh4_levels(refit2, ...) writes it, byte for byte; a
 * refused call (RT_E_*, rth_last_error()) leaves it alone. */
int rth_bvh4_refit(const RtBVHNode2* refit2, int32_t nNodes, int32_t nIdx, const uint32_t* roots, int32_t nRoots, RtBVHNode4* inout4,
                   const uint32_t* quadNode, int32_t nLive, int32_t* changedNodes);
/* rth_bvh4_refit on the scene's own arrays, after rth_refit: the scene's BVH4 must be the collapse of its BVH2 as it was before. */
int rth_refit_bvh4(RthScene* s, int32_t* changedNodes);
int rth_set_instance_transform(RthScene* s, int blas, const float invT[16]); /* scene.cpp:82 (commented out there) */
/* A further instance of the BLAS that instance `blas` renders: the new record (appended) carries that BLAS's root and invT (NULL: the
 * identity); its TLAS leaf gets its bounds from the next rth_build_tlas by the rule every instance's does (the root's box, mapped by
 * inverse(invT) unless invT is the identity).  What the host needs to state a scene with more instances than BLAS (rt_resize_scene's
 * ground truth).  Returns the new instance's index, or -1: a bad index, a singular invT, 256 instances already. */
int rth_add_instance(RthScene* s, int blas, const float invT[16]);
/* Instances a and b trade places (record for record): the order of the instances is free, and the derived pair ids follow the order in
 * which the instances first name their BLAS, not the order of the BLAS.  -1: a bad index. */
int rth_swap_instances(RthScene* s, int a, int b);
/* The light list of prims[nPrims] under mats[nMats] by the Scene rule, as rt_resize_scene derives it (csrc/resize_common.h): the
 * indices, in increasing order, of the primitives whose material has isLight != 0.  out needs room for nPrims entries; returns the
 * count, or RT_E_INVALID for a missing array or the first primitive whose objType / matIdx is out of range (rth_last_error() names it). */
int rth_light_list(const RtPrimitive* prims, int32_t nPrims, const RtMaterial* mats, int32_t nMats, uint32_t* out);
/* The host restatement of rt_update_materials (rt355.h), one call per part, with the same checks (csrc/resize_common.h):
 *   rth_set_materials       replaces the whole table; every texture window must lie inside the atlas and every primitive's matIdx
 *                           inside the new table (names of materials the new table drops are forgotten);
 *   rth_set_texels          gives the atlas nTexels texels (-1: as it is; kept texels stay, new ones are zero; the table must still fit)
 *                           and writes texels[count] at [first, first + count) (texels NULL: nothing is written);
 *   rth_set_prim_materials  writes matIdx[count] into primitives [first, first + count), each inside the table.
 * Afterwards the scene's light list is the Scene rule's for the new state (the indices, in increasing order, of the primitives whose
 * material has isLight != 0); the trees are not touched.  Each returns RT_E_INVALID (rth_last_error() has the reason) and changes nothing
 * when it refuses. */
int rth_set_materials(RthScene* s, const RtMaterial* mats, int32_t nMats);
int rth_set_texels(RthScene* s, const RtFloat4* texels, int32_t first, int32_t count, int32_t nTexels);
int rth_set_prim_materials(RthScene* s, int32_t first, int32_t count, const int32_t* matIdx);

/* Borrowed views of the arrays (valid until the scene changes). */
const RtPrimitive*   rth_primitives(RthScene* s, int* n);
const RtMaterial*    rth_materials(RthScene* s, int* n);
const RtFloat4*      rth_textures(RthScene* s, int* n);
const uint32_t*      rth_lights(RthScene* s, int* n);
const RtBVHNode2*    rth_bvh2_nodes(RthScene* s, int* n);
const RtBVHNode4*    rth_bvh4_nodes(RthScene* s, int* n);
const uint32_t*      rth_prim_idx(RthScene* s, int* n);
const RtTLASNode*    rth_tlas_nodes(RthScene* s, int* n);
const RtBVHInstance* rth_blas_nodes(RthScene* s, int* n);
/* BVH statistics (bvh.h:21-22): depth, node count, spatial splits, clipped prims, prim count, SAH cost, build ms. */
int rth_bvh_stats(RthScene* s, uint32_t out_u[5], float out_f[2]);

/* CameraManager(vfov,type) + origin/forward/aperture/focalLength + UpdateCamVec() (camera.h:24-34,101-121). */
int rth_camera(int width, int height, float vfov, int type, const float origin[3], const float forward[3],
               float aperture, float focalLength, RtCamera* out);

/* seeds[i] = (first+i+1)-th xorshift32 output from 0x12345678: the host seed loop of renderer.cpp:195-196
 * (RandomUInt, template/template.cpp:711,724-730), with a start offset for row bands / sample partitions. */
int rth_seed_stream(uint32_t* out, int64_t first, int64_t n);

/* Renderer mirror (renderer.cpp:6-63): owns a context of librt355.so. */
RthRenderer* rth_renderer_create(RthScene* scene /* adopted */, int width, int height, int device, int y0, int y1,
                                 int shading, int sampling, int bvh, int russianRoulette, int filterFireflies);
void rth_renderer_destroy(RthRenderer* r);
int  rth_renderer_init(RthRenderer* r);                                   /* Renderer::Init  */
int  rth_renderer_set_camera(RthRenderer* r, const float origin[3], const float forward[3], float fov, float aperture);
int  rth_renderer_tick(RthRenderer* r, int frames);                       /* Renderer::Tick x frames */
int  rth_renderer_read(RthRenderer* r, RtFloat4* out, float* energy);     /* accumBuffer read-back + ComputeEnergy */
int  rth_renderer_camera(RthRenderer* r, RtCamera* out);
int  rth_renderer_save_frame(RthRenderer* r, const char* file);
/* CameraManager::Move / MouseMove / Zoom (camera.h:47-99); the next Tick() sees camera.moved and resets (renderer.cpp:41-46). */
int  rth_renderer_camera_move(RthRenderer* r, int camdir /* 0 Forward 1 Backwards 2 Left 3 Right 4 Up 5 Down */);
int  rth_renderer_camera_mouse(RthRenderer* r, float xOffset, float yOffset);
int  rth_renderer_camera_zoom(RthRenderer* r, float offset);
int rth_renderer_set_lanes(RthRenderer* r, int lanes);   /* before rth_renderer_init: Renderer::lanes (Tick = `lanes` overlapping frames) */
int rth_renderer_set_builtins(RthRenderer* r, int builtins);   /* before rth_renderer_init: Renderer::builtins = RtConfig.builtins of the lanes (RT_BUILTINS_*, rt355.h); other values: -1 */
int rth_renderer_builtins(RthRenderer* r);                /* the stored setting (RT_BUILTINS_DEFAULT until set) */
int  rth_renderer_frames(RthRenderer* r);                                 /* settings->frames */          /* Renderer::SaveFrame (renderer.cpp:303-308) */

#ifdef __cplusplus
}
#endif
#endif

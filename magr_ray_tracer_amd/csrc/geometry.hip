// geometry.hip — the two kernels behind an RtGeometry whose data lie on the device (include/rt355.h; driven by scene_rebuild.hip's
// stage_geometry; rules: geometry_common.h):
//   k_window_check        records form: one thread per record of the window, objType / matIdx against the bound record
//   k_tri_from_vertices   vertex form: one thread per triangle of the window, the rows that follow from three positions
// Both report the lowest offending index of the window through atomicMin into a status word that starts at geometry's kNoBad.
#include <hip/hip_runtime.h>
#include "geometry_common.h"
#include "geometry_dev.h"

namespace {
constexpr int kBlock = 256;
dim3 grid(uint32_t n) { return dim3((n + kBlock - 1) / kBlock); }
}

// given[i] replaces bound[i] (both start at the window): its objType and matIdx must be the bound ones.  Holders only read `bound`.
__global__ void __launch_bounds__(kBlock) k_window_check(const RtPrimitive* given, const RtPrimitive* bound, uint32_t count, uint32_t* bad)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    const int2 g = *reinterpret_cast<const int2*>(&given[i].objType), b = *reinterpret_cast<const int2*>(&bound[i].objType);
    if (g.x != b.x || g.y != b.y) atomicMin(bad, i);   // a value, not a position
}

// staged[i] (the window of the staged copy of the bound primitives) moves to three positions: vertex j's x, y, z are the dwords at
// positions + j * strideDwords.  The five rows are vector stores; the positions are dword loads, since a stride of 12 bytes has no wider
// alignment.  An index that is no vertex is never followed: the record stays as staged and the triangle is reported.
__global__ void __launch_bounds__(kBlock) k_tri_from_vertices(RtPrimitive* staged, uint32_t count, const float* positions, uint64_t strideDwords, uint64_t nVertices,
                                                              const uint32_t* indices, uint32_t* bad)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    uint64_t j0 = 3ull * i, j1 = j0 + 1, j2 = j0 + 2;
    if (indices) { j0 = indices[j0]; j1 = indices[j1]; j2 = indices[j2]; }
    if (j0 >= nVertices || j1 >= nVertices || j2 >= nVertices) { atomicMin(bad, i); return; }
    const int64_t strideBytes = (int64_t)(strideDwords * 4);
    const geometry::V3 a = geometry::vertex(positions, strideBytes, j0), b = geometry::vertex(positions, strideBytes, j1), c = geometry::vertex(positions, strideBytes, j2);
    RtFloat4* rows = reinterpret_cast<RtFloat4*>(staged + i);   // v0, v1, v2, N, centroid: the record's first five rows
    const float4* in = reinterpret_cast<const float4*>(rows);
    const float4 b0 = in[0], b1 = in[1], b2 = in[2], bN = in[3];
    const bool flip = geometry::flipped(RtFloat4{ bN.x, bN.y, bN.z, bN.w }, RtFloat4{ b0.x, b0.y, b0.z, b0.w }, RtFloat4{ b1.x, b1.y, b1.z, b1.w },
                                        RtFloat4{ b2.x, b2.y, b2.z, b2.w });
    const geometry::TriRows t = geometry::tri_rows(a, b, c, flip);
    float4* out = reinterpret_cast<float4*>(rows);
    out[0] = make_float4(t.v0.x, t.v0.y, t.v0.z, t.v0.w);
    out[1] = make_float4(t.v1.x, t.v1.y, t.v1.z, t.v1.w);
    out[2] = make_float4(t.v2.x, t.v2.y, t.v2.z, t.v2.w);
    out[3] = make_float4(t.N.x, t.N.y, t.N.z, t.N.w);
    out[4] = make_float4(t.centroid.x, t.centroid.y, t.centroid.z, t.centroid.w);
    staged[i].area = t.area;
}

namespace geometrydev {

hipError_t window_check(hipStream_t s, const RtPrimitive* given, const RtPrimitive* bound, uint32_t count, uint32_t* bad)
{
    hipError_t e = hipMemsetAsync(bad, 0xff, sizeof(uint32_t), s);   // kNoBad
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_window_check, grid(count), dim3(kBlock), 0, s, given, bound, count, bad);
    return hipGetLastError();
}
hipError_t tri_from_vertices(hipStream_t s, RtPrimitive* staged, uint32_t count, const float* positions, int64_t strideBytes, int64_t nVertices,
                             const uint32_t* indices, uint32_t* bad)
{
    hipError_t e = hipMemsetAsync(bad, 0xff, sizeof(uint32_t), s);   // kNoBad
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_tri_from_vertices, grid(count), dim3(kBlock), 0, s, staged, count, positions, (uint64_t)strideBytes / 4, (uint64_t)nVertices, indices, bad);
    return hipGetLastError();
}

} // namespace geometrydev

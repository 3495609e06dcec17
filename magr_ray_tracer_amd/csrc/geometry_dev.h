// geometry_dev.h — the interface between scene_rebuild.hip's stage_geometry and geometry.hip's kernels (rules: geometry_common.h).
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/rt355_types.h"

namespace geometrydev {
constexpr uint32_t kNoBad = 0xffffffffu;   // the status word while nothing of the window has been refused
// Records form: given[0, count) against bound[0, count) (both device-reachable, both at the window's start); *bad receives the lowest
// index whose objType or matIdx differs
hipError_t window_check(hipStream_t s, const RtPrimitive* given, const RtPrimitive* bound, uint32_t count, uint32_t* bad);
// Vertex form: staged[0, count) (the window of the staged primitives) from positions (device-reachable, nVertices vertices strideBytes
// apart) through indices (device-reachable, 3 * count of them; NULL: 3i, 3i + 1, 3i + 2); *bad receives the lowest triangle with an
// index >= nVertices (such a record stays as staged)
hipError_t tri_from_vertices(hipStream_t s, RtPrimitive* staged, uint32_t count, const float* positions, int64_t strideBytes, int64_t nVertices,
                             const uint32_t* indices, uint32_t* bad);
}

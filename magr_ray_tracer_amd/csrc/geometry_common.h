// geometry_common.h — the one statement of how a triangle record follows from three vertex positions (RtGeometry's vertex form,
// include/rt355.h), compiled by hipcc for the device path (geometry.hip's k_tri_from_vertices) and by g++ for the host mirror
// (host/host_capi.cpp, rth_set_vertices), and the checks of an RtGeometry that need no device (rt_geometry_check, rth_set_vertices).
//
// The rule is Scene::AddTriangle's (host/scene_build.cpp), word for word:
//   v0, v1, v2   the positions as to4 writes them (w 0)
//   N            normalize(cross(v1 - v0, v2 - v0)) with the host's normalize: 1.0f / sqrtf(dot), then the product; w 0
//   centroid     (v0 + v1 + v2) * (1 / 3.f), in that order; w 0
//   area         Heron's formula over length(v1 - v0), length(v1 - v2), length(v2 - v0)
// AddTriangle's `flip` is not stored in a record, so the sign is carried over from the bound one: the new N is negated (all four words,
// as AddTriangle negates them) iff dot(bound N, cross(bound v1 - bound v0, bound v2 - bound v0)) < 0.  The comparison is false for zero
// and NaN: a bound triangle without a normal counts as not flipped.
// A triangle whose cross product is zero or not finite gets NaN in N, and may get NaN in area (Heron under a negative rounding error);
// x86 and the GPU make NaNs of different sign, so for those words the promise is "NaN where the host has NaN".
//
// Where the rule holds (tests/geometry_check.py: a ladder of triangles with smallest angle >= 10 degrees at every power of two; host and
// GPU agree in every regime).  Edges of about 2^-32 .. 2^31: a unit N and a finite positive area; against float64 | |N| - 1 | < 3.2e-7,
// the angle to the true normal < 5.9e-7 rad, the centroid within 3.4 ulps of the largest coordinate, the area within 9.9e-6 relative.
// Smaller: dot(cross, cross) is subnormal (edges 2^-38 .. 2^-33: N finite, no unit vector), then 0 (2^-76 .. 2^-38: 1 / sqrtf is inf, N
// holds inf and NaN, area 0), then the cross product is 0 (below 2^-75, points, exactly collinear vertices: N NaN, area 0).  Larger:
// dot(cross, cross) overflows (2^32 .. 2^63: N is (0, 0, 0), area inf), then cross and the lengths (from 2^63: N and area NaN).  The
// centroid is inf where the sum of three coordinates overflows, whatever N and area are; v0, v1, v2 are the caller's bits always.
// A triangle that passes through a state whose N is NaN or zero has lost its flip: the next call reads it as not flipped.
//
// Floating point: strict binary32 in source order (-ffp-contract=off on both sides), division and sqrtf correctly rounded on both sides.
#pragma once
#include <stdint.h>
#include <math.h>
#include <string>
#include "../../include/rt355.h"
#include "lbvh_common.h"

namespace geometry {

struct V3 { float x, y, z; };
LB_HD V3 v3(float x, float y, float z) { V3 r; r.x = x; r.y = y; r.z = z; return r; }
LB_HD V3 v3(const RtFloat4& a) { return v3(a.x, a.y, a.z); }
LB_HD V3 sub(const V3& a, const V3& b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
LB_HD V3 add(const V3& a, const V3& b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
LB_HD V3 mul(const V3& a, float s) { return v3(a.x * s, a.y * s, a.z * s); }
LB_HD float dot(const V3& a, const V3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
LB_HD V3 cross(const V3& a, const V3& b) { return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
LB_HD float length(const V3& v) { return sqrtf(dot(v, v)); }
LB_HD V3 normalize(const V3& v) { const float inv = 1.0f / sqrtf(dot(v, v)); return mul(v, inv); }
LB_HD RtFloat4 to4(const V3& v) { RtFloat4 r; r.x = v.x; r.y = v.y; r.z = v.z; r.w = 0.0f; return r; }

// the words of a triangle record that follow from its vertices
struct TriRows { RtFloat4 v0, v1, v2, N, centroid; float area; };

// AddTriangle's flip, read back from a bound record
LB_HD bool flipped(const RtFloat4& N, const RtFloat4& v0, const RtFloat4& v1, const RtFloat4& v2)
{
    return dot(v3(N), cross(sub(v3(v1), v3(v0)), sub(v3(v2), v3(v0)))) < 0.0f;
}
// the rows of the triangle (a, b, c); flip: AddTriangle's
LB_HD TriRows tri_rows(const V3& a, const V3& b, const V3& c, bool flip)
{
    TriRows t;
    t.v0 = to4(a); t.v1 = to4(b); t.v2 = to4(c);
    t.N = to4(normalize(cross(sub(b, a), sub(c, a))));
    if (flip) { t.N.x *= -1; t.N.y *= -1; t.N.z *= -1; t.N.w *= -1; }
    t.centroid = to4(mul(add(add(a, b), c), 1 / 3.f));
    const float la = length(sub(b, a)), lb = length(sub(b, c)), lc = length(sub(c, a));
    const float s = 0.5f * (la + lb + lc);
    t.area = sqrtf(s * (s - la) * (s - lb) * (s - lc));
    return t;
}
// vertex j of a position array of dwords: x, y, z at byte offset j * strideBytes (a stride of 12 has no wider alignment)
LB_HD V3 vertex(const float* positions, int64_t strideBytes, uint64_t j)
{
    const float* p = positions + j * (uint64_t)(strideBytes / 4);
    return v3(p[0], p[1], p[2]);
}
// the bound record p moved to the vertices (a, b, c): the five rows and the area anew, uv*, objType, matIdx and the pad words as they are
inline void set_triangle(RtPrimitive& p, const V3& a, const V3& b, const V3& c)
{
    RtTriangle& t = p.obj.triangle;
    const TriRows r = tri_rows(a, b, c, flipped(t.N, t.v0, t.v1, t.v2));
    t.v0 = r.v0; t.v1 = r.v1; t.v2 = r.v2; t.N = r.N; t.centroid = r.centroid;
    p.area = r.area;
}

// ---- host only: the checks of an RtGeometry that need no device (nPrims primitives are bound) ----------------------------------------
// RT_OK, or RT_E_INVALID with msg (without the caller's name).  primType (nPrims entries, NULL: all triangles) is read in vertex form only.
inline int check_args(const RtGeometry* g, int64_t nPrims, const int32_t* primType, std::string& msg)
{
    if (!g) { msg = "null geometry"; return RT_E_INVALID; }
    // (the first three in the words rt_update_scene has always used)
    if (g->count < 0 || (g->count > 0 && !g->prims && !g->positions)) { msg = "bad primitive count " + std::to_string(g->count) + " / NULL records"; return RT_E_INVALID; }
    if (g->count == 0) {
        if (g->first < 0) { msg = "the window starts at primitive " + std::to_string(g->first); return RT_E_INVALID; }
        return RT_OK;
    }
    if (g->first < 0 || (int64_t)g->first + g->count > nPrims) {
        msg = "primitive range [" + std::to_string(g->first) + ", " + std::to_string((int64_t)g->first + g->count) + ") outside the " + std::to_string(nPrims) + " uploaded";
        return RT_E_INVALID;
    }
    if (g->prims && g->positions) { msg = "both prims and positions are given: exactly one source of geometry is taken"; return RT_E_INVALID; }
    if (g->prims) return RT_OK;
    if (g->positionStride < 12 || g->positionStride % 4) {
        msg = "positionStride " + std::to_string(g->positionStride) + ": at least 12 bytes and a multiple of 4 are required";
        return RT_E_INVALID;
    }
    if (g->nVertices < 0) { msg = "nVertices " + std::to_string(g->nVertices) + " is negative"; return RT_E_INVALID; }
    if (!g->indices && g->nVertices < 3 * (int64_t)g->count) {
        msg = std::to_string(g->nVertices) + " vertices for " + std::to_string(g->count) + " triangles without indices: " + std::to_string(3 * (int64_t)g->count) + " are needed";
        return RT_E_INVALID;
    }
    if (primType) for (int64_t i = g->first; i < (int64_t)g->first + g->count; i++) if (primType[i] != RT_PRIM_TRIANGLE) {
        msg = "primitive " + std::to_string(i) + " is no triangle (objType " + std::to_string(primType[i]) + "): the vertex form moves triangles only";
        return RT_E_INVALID;
    }
    return RT_OK;
}
// the refusal of an index that is no vertex: triangle `tri` of the window, its three indices
inline std::string bad_index_message(int64_t tri, const uint32_t idx[3], int64_t nVertices)
{
    int k = 0;
    while (k < 2 && (int64_t)idx[k] < nVertices) k++;
    return "triangle " + std::to_string(tri) + " of the window: index " + std::to_string(idx[k]) + " (corner " + std::to_string(k) + ") is no vertex, nVertices is " + std::to_string(nVertices) +
           "; the scene is unchanged";
}

} // namespace geometry

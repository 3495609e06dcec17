/* oracle.c — TEST INFRASTRUCTURE ONLY (see oracle.h).
 *
 * Plain-C restatement of the reference's wavefront hot path.  Every function names
 * the reference lines it follows (paths relative to the reference repository).
 *
 * Float discipline (what "the reference result" means here): the arithmetic of the
 * reference's OpenCL C source as the ROCm 7.2 OpenCL compiler builds it for gfx950
 * WITHOUT fast-math (-O2 -ffp-contract=off -cl-fp32-correctly-rounded-divide-sqrt,
 * see oracle/build_ref.sh): source-level + - * / are separate IEEE binary32
 * operations; the builtins dot() and cross() are the fused-multiply-add chains of
 * ROCm's OpenCL library (dot: x*x' then fma y, z, w; cross: fma(a.y,b.z,-(a.z*b.y)));
 * length() and normalize() carry that library's rescaling branches; min/max are
 * minNum/maxNum.  ONE deliberate difference: the library's normalize() multiplies by
 * the hardware reciprocal square root (v_rsq_f32, 1 ulp, not reproducible off the
 * GPU); here and in the HIP path it is v * (1.0f / sqrtf(d)) with IEEE sqrt and
 * divide, so directions can differ from the reference build in the last 1-2 ulp.
 * Transcendentals (sin, cos, exp, acospi, atan2pi: fisheye camera, sphere lights,
 * sphere textures, dielectrics) are NOT libm calls: they are the single-precision Cephes
 * algorithms written out as IEEE + - * / sqrt (orc_expf ... below), the same sequences
 * the HIP path evaluates, so those scenes are bit-exact HIP vs oracle too; against the
 * reference's device-library builtins they are a few ulp off (like normalize).
 * float -> int conversions follow the GPU (NaN -> 0, saturating; f2i_gpu).
 *
 * Build: gcc -O2 -ffp-contract=off -mfma -fopenmp (magr_ray_tracer_amd/build.py build_oracle).
 */
#include "oracle.h"
#include "../include/rt355.h"   /* RT_MATH_* function ids */
#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

typedef RtFloat4 f4;

/* ---------------------------------------------------------------- vector helpers */
static inline f4 v4(float x, float y, float z, float w) { f4 r = { x, y, z, w }; return r; }
static inline f4 splat(float s) { return v4(s, s, s, s); }
static inline f4 add4(f4 a, f4 b) { return v4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
static inline f4 sub4(f4 a, f4 b) { return v4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
static inline f4 mul4(f4 a, f4 b) { return v4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
static inline f4 muls(f4 a, float s) { return v4(a.x * s, a.y * s, a.z * s, a.w * s); }
static inline f4 neg4(f4 a) { return v4(-a.x, -a.y, -a.z, -a.w); }
/* ROCm OpenCL library dot(float3/float4): x*x' then fma in y, z, (w) order. */
static inline float dot3(f4 a, f4 b) { return fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)); }
static inline float dot4(f4 a, f4 b) { return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x))); }
/* ROCm OpenCL library cross(float4): w = 0. */
static inline f4 cross4(f4 a, f4 b)
{
    return v4(fmaf(a.y, b.z, b.y * (-a.z)), fmaf(a.z, b.x, b.z * (-a.x)), fmaf(a.x, b.y, b.x * (-a.y)), 0.0f);
}
static inline float length4(f4 v)
{
    float d = dot4(v, v);
    if (d < FLT_MIN) { f4 s = muls(v, 0x1p+86f); return sqrtf(dot4(s, s)) * 0x1p-86f; }
    if (d == INFINITY) { f4 s = muls(v, 0x1p-66f); return sqrtf(dot4(s, s)) * 0x1p+66f; }
    return sqrtf(d);
}
static inline f4 normalize4(f4 v)
{
    if (v.x == 0.0f && v.y == 0.0f && v.z == 0.0f && v.w == 0.0f) return v;
    float d = dot4(v, v);
    if (d < FLT_MIN) { v = muls(v, 0x1p+86f); d = dot4(v, v); }
    else if (d == INFINITY) {
        v = muls(v, 0x1p-66f); d = dot4(v, v);
        if (d == INFINITY) {
            v = v4(copysignf(isinf(v.x) ? 1.0f : 0.0f, v.x), copysignf(isinf(v.y) ? 1.0f : 0.0f, v.y),
                   copysignf(isinf(v.z) ? 1.0f : 0.0f, v.z), copysignf(isinf(v.w) ? 1.0f : 0.0f, v.w));
            d = dot4(v, v);
        }
    }
    float r = 1.0f / sqrtf(d); /* reference build: v_rsq_f32 (file header) */
    return muls(v, r);
}

/* ---------------------------------------------------------------- transcendentals
 * exp (Beer's law), sin / cos (fisheye camera, sphere lights), acos / atan2 (sphere texture lookup) come from different math
 * libraries on a CPU and on the GPU (ROCm's device library leans on hardware v_exp / v_sin approximations), so calling libm here
 * and the device library there can never agree bit for bit - and a last-bit difference in a Fresnel draw or a texel index flips a
 * whole path.  Oracle and HIP path therefore both evaluate the SAME sequence of IEEE + - * / sqrt operations: the single-precision
 * Cephes algorithms (S. Moshier, cephes/single: expf.c, sinf.c, asinf.c, atanf.c - published coefficients and reduction constants),
 * each written out independently here and in rt355_kernels.h.  Against the reference's own kernels they differ by a few ulp, like
 * normalize() does; tests/test_gpu_reference.py bounds that. */
static inline float bits_f32(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static float orc_expf(float x)
{
    if (x != x) return x;
    if (x > 88.7228394f) return INFINITY;
    if (x < -103.972076f) return 0.0f;
    float n = floorf(x * 1.44269504088896341f + 0.5f);          /* round(x / ln 2) */
    float r = x - n * 0.693359375f;                              /* Cody-Waite: ln 2 = C1 + C2 */
    r = r - n * -2.12194440e-4f;
    float z = r * r;
    float p = 1.9875691500E-4f;
    p = p * r + 1.3981999507E-3f;
    p = p * r + 8.3334519073E-3f;
    p = p * r + 4.1665795894E-2f;
    p = p * r + 1.6666665459E-1f;
    p = p * r + 5.0000001201E-1f;
    float e = p * z;
    e = e + r;
    e = e + 1.0f;
    int k = (int)n;                                              /* e * 2^k in steps that stay representable */
    if (k > 127) { e = e * 0x1p127f; k -= 127; }
    else if (k < -126) { e = e * 0x1p-126f; k += 126; }
    return e * bits_f32((uint32_t)(k + 127) << 23);
}
/* argument reduction of sinf / cosf: octant j of |x| (made even-up), remainder in [-pi/4, pi/4] by three-term Cody-Waite */
static float orc_sincos_reduce(float ax, int* jOut)
{
    int j = (int)(1.27323954473516f * ax);                       /* 4 / pi */
    float y = (float)j;
    if (j & 1) { j += 1; y = y + 1.0f; }
    *jOut = j & 7;
    float r = ax - y * 0.78515625f;
    r = r - y * 2.4187564849853515625e-4f;
    r = r - y * 3.77489497744594108e-8f;
    return r;
}
static inline float orc_sin_poly(float x, float z) { float p = -1.9515295891E-4f * z + 8.3321608736E-3f; p = p * z - 1.6666654611E-1f; p = p * z; p = p * x; return p + x; }
static inline float orc_cos_poly(float z) { float p = 2.443315711809948E-005f * z - 1.388731625493765E-003f; p = p * z + 4.166664568298827E-002f; p = p * z; p = p * z; p = p - 0.5f * z; return p + 1.0f; }
static float orc_sinf(float x)
{
    if (x != x) return x;
    int neg = x < 0.0f; float ax = neg ? -x : x;
    if (x == 0.0f) return x;                                     /* sin(-0) = -0 */
    if (ax == INFINITY) return x - x;                            /* NaN */
    if (ax > 8192.0f) return 0.0f;                               /* total loss of precision (cephes) */
    int j; float r = orc_sincos_reduce(ax, &j);
    if (j > 3) { neg = !neg; j -= 4; }
    float z = r * r;
    float y = (j == 1 || j == 2) ? orc_cos_poly(z) : orc_sin_poly(r, z);
    return neg ? -y : y;
}
static float orc_cosf(float x)
{
    if (x != x) return x;
    float ax = x < 0.0f ? -x : x;
    if (ax == INFINITY) return x - x;                            /* NaN */
    if (ax > 8192.0f) return 0.0f;
    int j; float r = orc_sincos_reduce(ax, &j);
    int neg = 0;
    if (j > 3) { neg = !neg; j -= 4; }
    if (j > 1) neg = !neg;
    float z = r * r;
    float y = (j == 1 || j == 2) ? orc_sin_poly(r, z) : orc_cos_poly(z);
    return neg ? -y : y;
}
static float orc_asinf(float x)                                   /* |x| <= 1 */
{
    int neg = x < 0.0f; float a = neg ? -x : x;
    if (a > 1.0f) return (x - x) / (x - x);                      /* NaN */
    if (a < 1.0e-4f) return x;
    float z, w; int flag = 0;
    if (a > 0.5f) { z = 0.5f * (1.0f - a); w = sqrtf(z); flag = 1; }
    else { w = a; z = w * w; }
    float p = 4.2163199048E-2f * z + 2.4181311049E-2f;
    p = p * z + 4.5470025998E-2f;
    p = p * z + 7.4953002686E-2f;
    p = p * z + 1.6666752422E-1f;
    p = p * z;
    p = p * w;
    p = p + w;
    if (flag) { p = p + p; p = 1.5707963267948966192f - p; }
    return neg ? -p : p;
}
static float orc_acosf(float x)
{
    if (x != x) return x;
    if (x < -1.0f || x > 1.0f) return (x - x) / (x - x);         /* NaN: a non-unit sphere normal (w-lane pollution) gets here */
    if (x < -0.5f) return 3.14159265358979323846f - 2.0f * orc_asinf(sqrtf(0.5f * (1.0f + x)));
    if (x > 0.5f) return 2.0f * orc_asinf(sqrtf(0.5f * (1.0f - x)));
    return 1.5707963267948966192f - orc_asinf(x);
}
static float orc_atanf(float x)
{
    int neg = signbit(x) != 0; float a = neg ? -x : x, y;
    if (a > 2.414213562373095f) { y = 1.5707963267948966192f; a = -(1.0f / a); }
    else if (a > 0.4142135623730950f) { y = 0.7853981633974483096f; a = (a - 1.0f) / (a + 1.0f); }
    else y = 0.0f;
    float z = a * a;
    float p = 8.05374449538e-2f * z - 1.38776856032E-1f;
    p = p * z + 1.99777106478E-1f;
    p = p * z - 3.33329491539E-1f;
    p = p * z;
    p = p * a;
    p = p + a;
    y = y + p;
    return neg ? -y : y;
}
static float orc_atan2f(float y, float x)
{
    if (x != x || y != y) return x + y;
    if (x == 0.0f) {
        if (y == 0.0f) return signbit(x) ? copysignf(3.14159265358979323846f, y) : y;
        return y > 0.0f ? 1.5707963267948966192f : -1.5707963267948966192f;
    }
    if (isinf(x) && isinf(y)) return copysignf(x > 0.0f ? 0.7853981633974483096f : 2.3561944901923449288f, y);
    float z = orc_atanf(y / x);
    if (x < 0.0f) z = signbit(y) ? z - 3.14159265358979323846f : z + 3.14159265358979323846f;
    return z;
}

/* ---------------------------------------------------------------- RNG (util.cl:50-59) */
uint32_t orc_xorshift32(uint32_t* s)
{
    uint32_t x = *s;
    x ^= x << 13; x ^= x >> 17; x ^= x << 5;
    *s = x;
    return x;
}
static inline float rnd_float(uint32_t* s) { return (float)orc_xorshift32(s) * 2.3283064365387e-10f; } /* util.cl:57 */
static inline float rnd_abs(uint32_t* s) { return fabsf(rnd_float(s)); }                                 /* util.cl:58 */
static inline f4 rnd_float3(uint32_t* s) { float x = rnd_float(s), y = rnd_float(s), z = rnd_float(s); return v4(x, y, z, 0.0f); } /* util.cl:59 */

/* Host seed stream: seeds[i] = (first+i+1)-th xorshift32 output from 0x12345678
 * (renderer.cpp:195-196, template/template.cpp:711,724-730). */
void orc_seed_stream(uint32_t* seeds, int64_t first, int64_t n)
{
    uint32_t s = 0x12345678u;
    for (int64_t i = 0; i < first; i++) orc_xorshift32(&s);
    for (int64_t i = 0; i < n; i++) seeds[i] = orc_xorshift32(&s);
}

/* ---------------------------------------------------------------- rays (ray.cl) */
static inline void init_ray(RtRay* r, f4 O, f4 D) /* ray.cl:4-19; pixelIdx,u,v stay as they are */
{
    r->O = O; r->D = D;
    r->rD = v4(1.0f / D.x, 1.0f / D.y, 1.0f / D.z, 1.0f / D.w);
    r->N = splat(0.0f); r->I = splat(0.0f); r->intensity = splat(1.0f);
    r->t = 1e30f; r->primIdx = -1; r->bounces = 0; r->inside = 0; r->lastSpecular = 0;
}
static inline RtRay zero_ray(void) { RtRay r; memset(&r, 0, sizeof r); return r; }

static RtRay reflect_ray(const RtRay* ray) /* ray.cl:21-29 */
{
    float dnd = dot4(ray->N, ray->D);
    f4 reflected = sub4(ray->D, muls(muls(ray->N, 2.0f), dnd));   /* D - (2*N)*dot */
    f4 origin = add4(ray->I, muls(muls(reflected, 2.0f), RT_EPSILON)); /* I + (reflected*2)*EPSILON */
    RtRay r = zero_ray(); init_ray(&r, origin, reflected);
    r.intensity = ray->intensity; r.bounces = ray->bounces + 1;
    return r;
}
static RtRay transmit_ray(const RtRay* ray, f4 T) /* ray.cl:31-39 */
{
    f4 origin = add4(ray->I, muls(T, RT_EPSILON));
    RtRay r = zero_ray(); init_ray(&r, origin, T);
    r.intensity = ray->intensity; r.bounces = ray->bounces + 1; r.inside = !ray->inside;
    return r;
}
static f4 sample_ball(uint32_t* seed) /* ray.cl:49-53 / 62-69: reject outside the unit ball (xyz); w = -1 */
{
    f4 p = sub4(muls(rnd_float3(seed), 2.0f), splat(1.0f));
    while (p.x * p.x + p.y * p.y + p.z * p.z > 1.0f) p = sub4(muls(rnd_float3(seed), 2.0f), splat(1.0f));
    return normalize4(p);
}
static f4 random_ray_hemisphere(f4 N, uint32_t* seed) /* ray.cl:46-56 */
{
    f4 p = sample_ball(seed);
    return dot4(N, p) < 0.0f ? neg4(p) : p;
}
static f4 cosine_ray_hemisphere(f4 N, uint32_t* seed) /* ray.cl:59-72 */
{
    f4 p = sample_ball(seed);
    return normalize4(add4(N, p));
}

/* ---------------------------------------------------------------- camera (camera.cl) */
static void primary_ray(RtRay* r, int x, int y, const RtCamera* cam, int aa, int W, int H, uint32_t* seed) /* camera.cl:6-46 */
{
    if (cam->type == RT_CAM_PROJECTION) {
        float u = (float)x * (1.0f / (float)W);
        float v = (float)y * (1.0f / (float)H);
        if (aa) { u += rnd_float(seed) / (float)W; v += rnd_float(seed) / (float)H; }
        f4 P = add4(add4(cam->topLeft, muls(cam->horizontal, u)), muls(cam->vertical, v));
        f4 dir = normalize4(sub4(P, cam->origin));
        f4 focalPoint = add4(cam->origin, muls(dir, cam->focalLength));
        f4 O = add4(cam->origin, muls(sub4(rnd_float3(seed), splat(0.5f)), cam->aperture));
        dir = normalize4(sub4(focalPoint, O));
        init_ray(r, O, dir);
    } else { /* fisheye, camera.cl:25-44 */
        float u = ((float)x - (float)W * .5f) * (2.f / (float)W);
        float v = ((float)y - (float)H * .5f) * (2.f / (float)H);
        if (aa) { u += rnd_float(seed) / (float)W; v += rnd_float(seed) / (float)H; }
        float r2 = u * u + v * v;
        if (r2 > 1.0f) { init_ray(r, splat(0.0f), splat(0.0f)); return; }
        float rr = sqrtf(r2);
        float psi = rr * cam->fov * 3.14159265358979323846f / 180.0f; /* r*fov*M_PI_F/180 */
        float sinPsi = orc_sinf(psi), cosPsi = orc_cosf(psi);
        float sinAlpha = u / rr, cosAlpha = v / rr;
        f4 D = sub4(add4(muls(cam->up, sinPsi * cosAlpha), muls(cam->right, sinPsi * sinAlpha)), muls(cam->forward, cosPsi));
        init_ray(r, cam->origin, D);
    }
}
static void primary_ray_simple(RtRay* r, int x, int y, const RtCamera* cam, int W, int H) /* camera.cl:48-55 */
{
    float u = (float)x * (1.0f / (float)W);
    float v = (float)y * (1.0f / (float)H);
    f4 P = add4(add4(cam->topLeft, muls(cam->horizontal, u)), muls(cam->vertical, v));
    init_ray(r, cam->origin, normalize4(sub4(P, cam->origin)));
}

/* ---------------------------------------------------------------- primitives (primitives.cl) */
static void isect_sphere(int idx, const RtSphere* s, RtRay* ray) /* primitives.cl:11-30 */
{
    f4 oc = sub4(ray->O, s->pos);
    float b = dot4(oc, ray->D);
    float c = dot4(oc, oc) - s->r2;
    float t, d = b * b - c;
    if (d <= 0) return;
    d = sqrtf(d); t = -b - d;
    if (t < ray->t && t > 0) { ray->t = t; ray->primIdx = idx; return; }
    t = d - b;
    if (t < ray->t && t > 0) { ray->t = t; ray->primIdx = idx; return; }
}
static void isect_plane(int idx, const RtPlane* p, RtRay* ray) /* primitives.cl:32-44 */
{
    float t = -(dot4(ray->O, p->N) + p->d) / dot4(ray->D, p->N);
    if (t > ray->t || t < 0) return;
    ray->t = t; ray->primIdx = idx;
    f4 uAxis = v4(p->N.y, p->N.z, -p->N.x, 0.0f);
    f4 vAxis = cross4(uAxis, p->N);
    f4 I = add4(ray->O, muls(ray->D, ray->t));
    ray->u = dot4(I, uAxis); ray->v = dot4(I, vAxis);
}
static void isect_triangle(int idx, const RtTriangle* tri, RtRay* ray) /* primitives.cl:47-76 */
{
    f4 v0v1 = sub4(tri->v1, tri->v0);
    f4 v0v2 = sub4(tri->v2, tri->v0);
    f4 pvec = cross4(ray->D, v0v2);
    float det = dot4(v0v1, pvec);
    if (fabsf(det) < 1e-8f) return;
    float invDet = 1.0f / det;
    f4 tvec = sub4(ray->O, tri->v0);
    float u = dot4(tvec, pvec) * invDet;
    if (u < 0 || u > 1) return;
    f4 qvec = cross4(tvec, v0v1);
    float v = dot4(ray->D, qvec) * invDet;
    if (v < 0 || u + v > 1) return;
    float t = dot4(v0v2, qvec) * invDet;
    if (t > ray->t || t < 0) return;
    ray->t = t; ray->primIdx = idx; ray->u = u; ray->v = v;
}
static inline void isect_prim(int idx, const RtPrimitive* p, RtRay* ray) /* primitives.cl:78-89 */
{
    switch (p->objType) {
    case RT_PRIM_SPHERE:   isect_sphere(idx, &p->obj.sphere, ray); break;
    case RT_PRIM_PLANE:    isect_plane(idx, &p->obj.plane, ray); break;
    case RT_PRIM_TRIANGLE: isect_triangle(idx, &p->obj.triangle, ray); break;
    }
}
static f4 prim_normal(const RtPrimitive* p, f4 I) /* primitives.cl:91-105 */
{
    switch (p->objType) {
    case RT_PRIM_SPHERE: return muls(sub4(I, p->obj.sphere.pos), p->obj.sphere.invr);
    case RT_PRIM_PLANE:  return p->obj.plane.N;
    default:             return p->obj.triangle.N;
    }
}
static inline float fmod1(float x) { return fmodf(x, 1.f); }
/* float -> int as the GPU converts (v_cvt_i32_f32 / v_cvt_u32_f32: NaN -> 0, out of range saturates).  OpenCL C leaves both
 * cases undefined and x86 returns INT_MIN for them; they DO occur on the path: a sphere hit found with w-lane-polluted dots
 *  has a non-unit normal, acospi(N.y) of |N.y| > 1 is NaN, and the reference's kernels (and the HIP path)
 * then read texel row 0.  Found by the whole-frame comparison with the reference's kernels (tests/test_gpu_reference.py). */
static inline int f2i_gpu(float x)
{
    if (x != x) return 0;
    if (x >= 2147483648.0f) return 2147483647;
    if (x <= -2147483648.0f) return (int)(-2147483647 - 1);
    return (int)x;
}
/* texel column / row of a sphere hit with normal N (primitives.cl:130-133); atan2pi with a double 0.5 */
static inline void orc_sphere_texel_xy(f4 N, int texW, int texH, int* x, int* y)
{
    float ux = (float)((1 + orc_atan2f(N.z, N.x) / 3.14159265358979323846) * 0.5);
    float uy = orc_acosf(N.y) / 3.14159265358979323846f;
    *x = f2i_gpu(ux * (float)texW);
    *y = f2i_gpu(uy * (float)texH);
}
static inline uint32_t f2u_gpu(float x)
{
    if (!(x > 0.0f)) return 0u;                 /* NaN and negatives */
    if (x >= 4294967296.0f) return 0xffffffffu;
    return (uint32_t)x;
}
/* The reference indexes `textures` unchecked (primitives.cl:124,134,145); texels outside the atlas are zero here and in the HIP path
 * (inside the atlas a stray index reads the neighbouring texture's texel, as the reference does). */
static inline f4 texel(const OrcScene* sc, long long i) { f4 z = { 0, 0, 0, 0 }; return i >= 0 && i < (long long)sc->nTex ? sc->tex[i] : z; }
static f4 albedo_of(const RtRay* ray, const OrcScene* sc) /* primitives.cl:107-148 */
{
    const RtPrimitive* prim = &sc->prims[ray->primIdx];
    const RtMaterial* mat = &sc->mats[prim->matIdx];
    f4 albedo = mat->color;
    if (mat->texIdx != -1) {
        switch (prim->objType) {
        case RT_PRIM_TRIANGLE: {
            const RtTriangle* t = &prim->obj.triangle;
            float w2 = 1 - ray->u - ray->v;
            float ux = fmod1(ray->u * t->uv1.x + ray->v * t->uv0.x + w2 * t->uv2.x);
            float uy = fmod1(ray->u * t->uv1.y + ray->v * t->uv0.y + w2 * t->uv2.y);
            if (ux < 0) ux = 1 + ux;
            if (uy < 0) uy = 1 + uy;
            int x = f2i_gpu(ux * (float)mat->texW), y = f2i_gpu(uy * (float)mat->texH);
            albedo = texel(sc, (long long)mat->texIdx + x + (long long)y * mat->texW);
        } break;
        case RT_PRIM_SPHERE: {
            int x, y;
            orc_sphere_texel_xy(ray->N, mat->texW, mat->texH, &x, &y);
            albedo = texel(sc, (long long)mat->texIdx + x + (long long)y * mat->texW);
        } break;
        case RT_PRIM_PLANE: {
            float u = fmod1(ray->u), v = fmod1(ray->v);
            if (u < 0) u = 1 - u;
            if (v < 0) v = 1 - v;
            int x = f2i_gpu(u * (float)mat->texW), y = f2i_gpu(v * (float)mat->texH);
            albedo = texel(sc, (long long)mat->texIdx + x + (long long)y * mat->texW);
        } break;
        }
    }
    return albedo;
}
static inline float survival_prob(f4 a) /* primitives.cl:150-153 */
{
    return fminf(fmaxf(fmaxf(a.x, fmaxf(a.y, a.z)), 0.f), 1.f);
}
static f4 random_point_on(const RtPrimitive* p, uint32_t* seed) /* primitives.cl:155-189 */
{
    if (p->objType == RT_PRIM_SPHERE) {
        const RtSphere* s = &p->obj.sphere;
        float theta = rnd_abs(seed) * 2.0f * 3.14159265358979323846f;
        float u = rnd_abs(seed) * 2.0f - 1.0f;
        float pre = sqrtf(1 - u * u);
        float x = orc_cosf(theta) * pre, y = orc_sinf(theta) * pre;
        return add4(muls(v4(x, y, u, 0.0f), s->r), s->pos);
    }
    const RtTriangle* t = &p->obj.triangle;
    float u1 = rnd_abs(seed), u2 = rnd_abs(seed);
    if (u1 + u2 > 1) { u1 = 1 - u1; u2 = 1 - u2; }
    f4 a = sub4(t->v1, t->v0), b = sub4(t->v2, t->v0);
    return add4(add4(t->v0, muls(a, u1)), muls(b, u2));
}

/* ---------------------------------------------------------------- traversal (bvh.cl, tlas.cl) */
static inline float isect_aabb(const RtRay* ray, f4 bmin, f4 bmax) /* bvh.cl:3-12 */
{
    float tx1 = (bmin.x - ray->O.x) * ray->rD.x, tx2 = (bmax.x - ray->O.x) * ray->rD.x;
    float tmin = fminf(tx1, tx2), tmax = fmaxf(tx1, tx2);
    float ty1 = (bmin.y - ray->O.y) * ray->rD.y, ty2 = (bmax.y - ray->O.y) * ray->rD.y;
    tmin = fmaxf(tmin, fminf(ty1, ty2)); tmax = fminf(tmax, fmaxf(ty1, ty2));
    float tz1 = (bmin.z - ray->O.z) * ray->rD.z, tz2 = (bmax.z - ray->O.z) * ray->rD.z;
    tmin = fmaxf(tmin, fminf(tz1, tz2)); tmax = fminf(tmax, fmaxf(tz1, tz2));
    if (tmax >= tmin && tmin < ray->t && tmax > 0) return tmin;
    return RT_REALLYFAR;
}
static int traverse_bvh2(RtRay* ray, const OrcScene* sc, uint32_t root, int occlusion, OrcCounters* c) /* bvh.cl:13-54 */
{
    const RtBVHNode2* nodes = sc->bvh2;
    const RtBVHNode2* stack[RT_BVH4_STACK]; /* reference: 32 (bvh.cl:15); 64 here so that deep SBVH trees cannot overflow */
    const RtBVHNode2* node = nodes + root;
    uint32_t sp = 0; int steps = 0;
    float t_light = ray->t;
    for (;;) {
        if (node->count > 0) {
            for (uint32_t i = 0; i < node->count; i++) {
                int index = (int)sc->primIdx[node->first + i];
                c->prim_tests++;
                isect_prim(index, &sc->prims[index], ray);
                if (occlusion && ray->t < t_light) return -1;
            }
            if (sp == 0) break;
            node = stack[--sp];
            continue;
        }
        c->node_visits++;
        const RtBVHNode2* c1 = &nodes[node->first];
        const RtBVHNode2* c2 = &nodes[node->first + 1];
        float d1 = isect_aabb(ray, c1->aabbMin, c1->aabbMax);
        float d2 = isect_aabb(ray, c2->aabbMin, c2->aabbMax);
        if (d1 > d2) { float d = d1; d1 = d2; d2 = d; const RtBVHNode2* t = c1; c1 = c2; c2 = t; }
        if (d1 >= t_light) {
            if (sp == 0) break;
            node = stack[--sp];
        } else {
            steps++;
            node = c1;
            if (d2 < t_light) { stack[sp++] = c2; steps++; }
        }
    }
    return steps;
}
/* The slab test of isect_aabb with both distances kept: the same six float32 products and minNum / maxNum chain, `hit` its visit
 * condition, *exitT the distance at which the ray leaves the box.  The pruning distance is ray->t, as in isect_aabb (bvh.cl:3-12) and in
 * the kernels' slab_any: in an occlusion traversal it is t_light until a primitive is accepted, and an accepted primitive ends the
 * traversal unless its t is not below t_light - equal to it, or a NaN (the triangle test rejects by comparisons, which a NaN passes).
 * After a NaN no box passes any more, here as in the reference's loop, whose failed box reports 1e30 >= t_light. */
static inline int slab_exit(const RtRay* ray, f4 bmin, f4 bmax, float* exitT)
{
    float tx1 = (bmin.x - ray->O.x) * ray->rD.x, tx2 = (bmax.x - ray->O.x) * ray->rD.x;
    float tmin = fminf(tx1, tx2), tmax = fmaxf(tx1, tx2);
    float ty1 = (bmin.y - ray->O.y) * ray->rD.y, ty2 = (bmax.y - ray->O.y) * ray->rD.y;
    tmin = fmaxf(tmin, fminf(ty1, ty2)); tmax = fminf(tmax, fmaxf(ty1, ty2));
    float tz1 = (bmin.z - ray->O.z) * ray->rD.z, tz2 = (bmax.z - ray->O.z) * ray->rD.z;
    tmin = fmaxf(tmin, fminf(tz1, tz2)); tmax = fminf(tmax, fmaxf(tz1, tz2));
    *exitT = tmax;
    return tmax >= tmin && tmin < ray->t && tmax > 0;
}
/* OrcConfig.connect_order == 1: the occlusion traversal of a BVH2 BLAS in the order the HIP path's connect uses (NOT the reference's).
 * Of the two children that pass the visit test the one the ray leaves LATER goes first - child 2 iff its exit distance is greater,
 * ties go to child 1 - and the other is pushed; with one passing child descend into it, with none pop.  Which nodes are reached at all
 * does not depend on the order, so neither does the verdict; the counts do.  (Two exceptions, on rays whose primitive tests are
 * float32 garbage - a direction component near FLT_MAX: a primitive accepted with a NaN t kills every later box, so the verdict depends
 * on which garbage primitive comes first; and for t_light > 1e30 the reference's loop above descends into boxes that failed - their 1e30
 * is below such a t_light - where this one, like the kernels' slab_any, does not.  tests/test_edge_rays_cpu.py pins the rays.)  Returns -1 for an occluded ray, else 0 (`steps` has no
 * reader in connect). */
static int traverse_bvh2_later_exit(RtRay* ray, const OrcScene* sc, uint32_t root, OrcCounters* c)
{
    const RtBVHNode2* nodes = sc->bvh2;
    const RtBVHNode2* stack[RT_BVH4_STACK];
    const RtBVHNode2* node = nodes + root;
    uint32_t sp = 0;
    const float t_light = ray->t;
    for (;;) {
        if (node->count > 0) {
            for (uint32_t i = 0; i < node->count; i++) {
                int index = (int)sc->primIdx[node->first + i];
                c->prim_tests++;
                isect_prim(index, &sc->prims[index], ray);
                if (ray->t < t_light) return -1;
            }
            if (sp == 0) break;
            node = stack[--sp];
            continue;
        }
        c->node_visits++;
        const RtBVHNode2* c1 = &nodes[node->first];
        const RtBVHNode2* c2 = &nodes[node->first + 1];
        float x1, x2;
        const int h1 = slab_exit(ray, c1->aabbMin, c1->aabbMax, &x1);
        const int h2 = slab_exit(ray, c2->aabbMin, c2->aabbMax, &x2);
        if (h1 && h2) {
            if (x2 > x1) { node = c2; stack[sp++] = c1; }
            else { node = c1; stack[sp++] = c2; }
        } else if (h1 || h2) {
            node = h1 ? c1 : c2;
        } else {
            if (sp == 0) break;
            node = stack[--sp];
        }
    }
    return 0;
}
static int traverse_bvh4(RtRay* ray, const OrcScene* sc, uint32_t root, int occlusion, OrcCounters* c) /* bvh.cl:55-96 */
{
    const RtBVHNode4* nodes = sc->bvh4;
    const RtBVHNode4* stack[RT_BVH4_STACK];
    const RtBVHNode4* node = nodes + root;
    uint32_t sp = 0; int steps = 0;
    float light_t = ray->t;
    for (;;) {
        steps++; c->node_visits++;
        float dist[4];
        for (int k = 0; k < 4; k++)
            dist[k] = node->first[k] != RT_INVALID ? isect_aabb(ray, node->aabbMin[k], node->aabbMax[k]) : RT_REALLYFAR;
        for (int k = 0; k < 4; k++) {
            if (node->first[k] == RT_INVALID) continue;
            if (dist[k] >= light_t) continue;
            if (node->count[k] > 0) {
                for (uint32_t j = 0; j < (uint32_t)node->count[k]; j++) {
                    int index = (int)sc->primIdx[node->first[k] + j];
                    c->prim_tests++;
                    isect_prim(index, &sc->prims[index], ray);
                    if (occlusion && ray->t < light_t) return -1;
                }
            } else {
                stack[sp++] = nodes + node->first[k];
            }
        }
        if (sp == 0) break;
        node = stack[--sp];
    }
    return steps;
}
static inline f4 xform_vec(f4 V, const float* T) /* util.cl:61-73 */
{
    return v4(dot3(v4(T[0], T[1], T[2], 0), V), dot3(v4(T[4], T[5], T[6], 0), V), dot3(v4(T[8], T[9], T[10], 0), V), 0.0f);
}
static inline f4 xform_pos(f4 V, const float* T) /* util.cl:75-87 */
{
    return v4(dot3(v4(T[0], T[1], T[2], 0), V) + T[3], dot3(v4(T[4], T[5], T[6], 0), V) + T[7],
              dot3(v4(T[8], T[9], T[10], 0), V) + T[11], 0.0f);
}
static int traverse_instance(RtRay* ray, const OrcScene* sc, const OrcConfig* cfg, const RtBVHInstance* inst, int occlusion, OrcCounters* c) /* tlas.cl:3-26 */
{
    f4 bO = ray->O, bD = ray->D, brD = ray->rD;
    float T[16]; memcpy(T, inst->invT, sizeof T);
    ray->D = xform_vec(bD, T);
    ray->O = xform_pos(bO, T);
    ray->rD = v4(1.0f / ray->D.x, 1.0f / ray->D.y, 1.0f / ray->D.z, 1.0f);
    c->inst_visits++;
    int steps = cfg->accel == ORC_ACCEL_BVH4 ? traverse_bvh4(ray, sc, inst->bvhIdx, occlusion, c)
              : occlusion && cfg->connect_order == ORC_CONNECT_LATER_EXIT ? traverse_bvh2_later_exit(ray, sc, inst->bvhIdx, c)
                                             : traverse_bvh2(ray, sc, inst->bvhIdx, occlusion, c);
    ray->D = bD; ray->O = bO; ray->rD = brD;
    return steps;
}
static int traverse_tlas(RtRay* ray, const OrcScene* sc, const OrcConfig* cfg, int occlusion, OrcCounters* c) /* tlas.cl:28-77 */
{
    const RtTLASNode* node = &sc->tlas[0];
    const RtTLASNode* stack[RT_TLAS_STACK];
    uint32_t sp = 0; int steps = 0;
    float t_light = ray->t;
    c->rays++;
    for (;;) {
        if (node->leftRight == 0) {
            int value = traverse_instance(ray, sc, cfg, &sc->blas[node->BLASidx], occlusion, c);
            if (occlusion && value == -1) return -1;
            steps += value;
            if (sp == 0) break;
            node = stack[--sp];
            continue;
        }
        c->tlas_visits++;
        const RtTLASNode* c1 = &sc->tlas[node->leftRight & 0xffff];
        const RtTLASNode* c2 = &sc->tlas[node->leftRight >> 16];
        float d1 = isect_aabb(ray, c1->aabbMin, c1->aabbMax);
        float d2 = isect_aabb(ray, c2->aabbMin, c2->aabbMax);
        if (d1 > d2) { float d = d1; d1 = d2; d2 = d; const RtTLASNode* t = c1; c1 = c2; c2 = t; }
        if (d1 >= t_light) {
            if (sp == 0) break;
            node = stack[--sp];
        } else {
            node = c1;
            if (d2 < t_light) stack[sp++] = c2;
        }
    }
    return steps;
}

/* ---------------------------------------------------------------- glass (glass.cl) */
static float fresnel(RtRay* ray, const RtMaterial* mat, f4* outT) /* glass.cl:4-49 */
{
    float costhetai = dot4(ray->N, muls(ray->D, -1.0f));
    float n1 = mat->n1, n2 = mat->n2;
    if (ray->inside) {
        n1 = mat->n2; n2 = mat->n1;
        ray->intensity.x *= orc_expf(-mat->absorption.x * ray->t); /* beersLaw, glass.cl:4-9 */
        ray->intensity.y *= orc_expf(-mat->absorption.y * ray->t);
        ray->intensity.z *= orc_expf(-mat->absorption.z * ray->t);
    }
    float frac = n1 * (1 / n2);
    float k = 1 - frac * frac * (1 - costhetai * costhetai);
    if (k < 0) return 1.f;
    *outT = normalize4(add4(muls(ray->D, frac), muls(ray->N, frac * costhetai - sqrtf(k))));
    float costhetat = dot4(neg4(ray->N), *outT);
    float n1ci = n1 * costhetai, n2ci = n2 * costhetai, n1ct = n1 * costhetat, n2ct = n2 * costhetat;
    float frac1 = (n1ci - n2ct) / (n1ci + n2ct);
    float frac2 = (n1ct - n2ci) / (n1ct + n2ci);
    float Fr = 0.5f * (frac1 * frac1 + frac2 * frac2);
    return mat->specular + (1 - mat->specular) * Fr;
}

/* ---------------------------------------------------------------- shading (shading.cl) */
#define PI_F   3.14159274101257f   /* M_PI_F   */
#define INVPI_F 0.31830987334251f  /* M_1_PI_F */

static f4 sample_dir(f4 N, uint32_t* seed, const OrcConfig* cfg)
{
    return cfg->sampling == ORC_SAMPLING_HEMISPHERE ? random_ray_hemisphere(N, seed) : cosine_ray_hemisphere(N, seed);
}
static f4 shade_kajiya(RtRay* ray, RtRay* ext, uint32_t* seed, const OrcScene* sc, const OrcConfig* cfg) /* shading.cl:7-70 */
{
    const RtPrimitive* prim = &sc->prims[ray->primIdx];
    const RtMaterial* mat = &sc->mats[prim->matIdx];
    if (mat->isLight) return mul4(ray->intensity, mat->emittance);
    RtRay r;
    float rnd = rnd_float(seed);
    if (mat->isDielectric) {
        f4 T = splat(0.0f);
        float Fr = fresnel(ray, mat, &T);
        r = rnd < Fr ? reflect_ray(ray) : transmit_ray(ray, T);
    } else if (rnd < mat->specular) {
        r = reflect_ray(ray);
    } else {
        f4 albedo = albedo_of(ray, sc);
        if (cfg->russian_roulette) {
            float rr_p = survival_prob(albedo);
            if (rr_p < rnd_float(seed)) return splat(0.0f);
            ray->intensity = muls(ray->intensity, 1 / rr_p);
        }
        f4 refl = sample_dir(ray->N, seed, cfg);
        float dotNR = dot4(ray->N, refl);
        float I_PDF = cfg->sampling == ORC_SAMPLING_HEMISPHERE ? 2 * PI_F : dotNR * PI_F;
        f4 BRDF = muls(albedo, INVPI_F);
        ray->intensity = mul4(ray->intensity, muls(muls(BRDF, I_PDF), dotNR)); /* intensity *= (BRDF*I_PDF)*dotNR */
        r = zero_ray(); init_ray(&r, add4(ray->I, muls(refl, RT_EPSILON)), refl);
        r.intensity = ray->intensity; r.bounces = ray->bounces + 1; r.inside = ray->inside;
    }
    r.pixelIdx = ray->pixelIdx;
    *ext = r;
    return splat(0.0f);
}
static f4 shade_nee(RtRay* ray, RtRay* ext, RtShadowRay* shadow, uint32_t* seed, const OrcScene* sc, const OrcConfig* cfg) /* shading.cl:72-169 */
{
    const RtPrimitive* prim = &sc->prims[ray->primIdx];
    const RtMaterial* mat = &sc->mats[prim->matIdx];
    if (mat->isLight) return ray->lastSpecular ? mul4(ray->intensity, mat->emittance) : splat(0.0f);
    RtRay r;
    float rnd = rnd_float(seed);
    if (mat->isDielectric) {
        f4 T = splat(0.0f);
        float Fr = fresnel(ray, mat, &T);
        r = rnd < Fr ? reflect_ray(ray) : transmit_ray(ray, T);
        r.lastSpecular = 1;
    } else if (rnd < mat->specular) {
        r = reflect_ray(ray);
        r.lastSpecular = 1;
    } else {
        f4 albedo = albedo_of(ray, sc);
        f4 BRDF = muls(albedo, INVPI_F);
        if (sc->nLights > 0) {
            /* reference reads lights[numLights] when the draw is exactly 1.0 (out of bounds,
             * probability 2^-25 per draw); both this oracle and the HIP path clamp instead. */
            uint32_t li = f2u_gpu(floorf(rnd_abs(seed) * (float)sc->nLights));
            if (li >= (uint32_t)sc->nLights) li = (uint32_t)sc->nLights - 1;
            uint32_t lightIdx = sc->lights[li];
            const RtPrimitive* lp = &sc->prims[lightIdx];
            f4 pl = random_point_on(lp, seed);
            f4 dirToLight = sub4(pl, ray->I);
            f4 Nl = prim_normal(lp, pl);
            float dist = length4(dirToLight);
            f4 L = muls(dirToLight, 1 / dist);
            float dotNL = dot4(ray->N, L);
            if (dotNL > 0 && dot4(Nl, neg4(L)) > 0) {
                shadow->I = ray->I; shadow->L = L; shadow->Nl = Nl;
                shadow->intensity = muls(ray->intensity, (float)sc->nLights);
                shadow->BRDF = BRDF; shadow->lightIdx = (int32_t)lightIdx; shadow->pixelIdx = ray->pixelIdx;
                shadow->dotNL = dotNL; shadow->dist = dist;
            }
        }
        if (cfg->russian_roulette) {
            float rr_p = survival_prob(albedo);
            if (rr_p < rnd_float(seed)) return splat(0.0f);
            ray->intensity = muls(ray->intensity, 1 / rr_p);
        }
        f4 refl = sample_dir(ray->N, seed, cfg);
        float dotNR = dot4(ray->N, refl);
        float I_PDF = cfg->sampling == ORC_SAMPLING_HEMISPHERE ? 2 * PI_F : dotNR * PI_F;
        r = zero_ray(); init_ray(&r, add4(ray->I, muls(refl, RT_EPSILON)), refl);
        r.intensity = muls(muls(mul4(ray->intensity, BRDF), I_PDF), dotNR); /* ((intensity*BRDF)*I_PDF)*dotNR */
        r.bounces = ray->bounces + 1; r.inside = ray->inside;
    }
    r.pixelIdx = ray->pixelIdx;
    *ext = r;
    return splat(0.0f);
}
static inline f4 firefly(f4 c, const OrcConfig* cfg) /* wavefront.cl:125-127,196-198 */
{
    if (cfg->filter_fireflies && dot4(c, c) > 25) return muls(normalize4(c), 5.0f);
    return c;
}

/* ---------------------------------------------------------------- kernels (wavefront.cl) */
void orc_generate(RtRay* rays, int32_t n, int32_t firstPixel, const OrcConfig* cfg, const RtCamera* cam,
                  int32_t aa, uint32_t* seeds) /* wavefront.cl:14-34 */
{
    for (int32_t i = 0; i < n; i++) {
        int32_t idx = firstPixel + i;
        RtRay r = zero_ray();
        primary_ray(&r, idx % cfg->width, idx / cfg->width, cam, aa, cfg->width, cfg->height, &seeds[i]);
        r.lastSpecular = 1; r.pixelIdx = idx;
        rays[i] = r;
    }
}
static void finish_hit(RtRay* ray, const OrcScene* sc) /* wavefront.cl:68-72 */
{
    if (ray->primIdx == -1) return;
    ray->I = add4(ray->O, muls(ray->D, ray->t));
    ray->N = prim_normal(&sc->prims[ray->primIdx], ray->I);
    if (dot4(ray->N, neg4(ray->D)) < 0) ray->N = muls(ray->N, -1.0f);
}
void orc_extend(RtRay* rays, int32_t n, const OrcScene* sc, const OrcConfig* cfg, int32_t renderBVH,
                RtFloat4* accum, int32_t* stepsOut, OrcCounters* ctr) /* wavefront.cl:35-75 */
{
    OrcCounters local; memset(&local, 0, sizeof local);
    for (int32_t idx = 0; idx < n; idx++) {
        RtRay* ray = &rays[idx];
        int steps = traverse_tlas(ray, sc, cfg, 0, &local);
        if (stepsOut) stepsOut[idx] = steps;
        if (renderBVH && accum) accum[idx] = splat((float)(uint32_t)steps / 255.f);
        finish_hit(ray, sc);
    }
    if (ctr) { ctr->rays += local.rays; ctr->tlas_visits += local.tlas_visits; ctr->inst_visits += local.inst_visits;
               ctr->node_visits += local.node_visits; ctr->prim_tests += local.prim_tests; }
}
void orc_shade(RtRay* in, int32_t nIn, RtRay* out, int32_t* nOut, RtShadowRay* shadow, int32_t* nShadow,
               const OrcScene* sc, const OrcConfig* cfg, RtFloat4* accum, uint32_t* seeds) /* wavefront.cl:76-142 */
{
    const f4 sky = v4(0.0784f, 0.0941f, 0.3215f, 0.0f); /* skydome.cl:7 */
    int s0 = cfg->schedule == ORC_SCHED_S0;
    for (int32_t k = 0; k < nIn; k++) {
        int32_t idx = s0 ? nIn - 1 - k : k;
        uint32_t* seed = s0 ? &seeds[0] : &seeds[idx];
        RtRay* ray = &in[idx];
        if (ray->primIdx == -1) {
            accum[ray->pixelIdx] = add4(accum[ray->pixelIdx], mul4(ray->intensity, sky));
            continue;
        }
        RtRay ext = zero_ray(); init_ray(&ext, splat(0.0f), splat(0.0f));
        ext.bounces = RT_MAX_BOUNCES + 1;
        RtShadowRay sr; memset(&sr, 0, sizeof sr); sr.pixelIdx = -1;
        f4 color = cfg->shading == ORC_SHADING_SIMPLE ? shade_kajiya(ray, &ext, seed, sc, cfg)
                                                      : shade_nee(ray, &ext, &sr, seed, sc, cfg);
        color = firefly(color, cfg);
        accum[ray->pixelIdx] = add4(accum[ray->pixelIdx], color);
        if (ext.bounces <= RT_MAX_BOUNCES) out[(*nOut)++] = ext;
        if (cfg->shading == ORC_SHADING_NEE && sr.pixelIdx != -1) shadow[(*nShadow)++] = sr;
    }
}
void orc_connect(const RtShadowRay* shadow, int32_t n, const OrcScene* sc, const OrcConfig* cfg,
                 RtFloat4* accum, OrcCounters* ctr) /* wavefront.cl:144-201 */
{
    OrcCounters local; memset(&local, 0, sizeof local);
    int s0 = cfg->schedule == ORC_SCHED_S0;
    for (int32_t k = 0; k < n; k++) {
        const RtShadowRay* s = &shadow[s0 ? n - 1 - k : k];
        RtRay ray = zero_ray();
        init_ray(&ray, add4(s->I, muls(s->L, RT_EPSILON)), s->L);
        ray.t = s->dist - 2 * RT_EPSILON;
        if (traverse_tlas(&ray, sc, cfg, 1, &local) == -1) continue;
        const RtPrimitive* lp = &sc->prims[s->lightIdx];
        float solidAngle = dot4(s->Nl, neg4(s->L)) * lp->area * (1 / (s->dist * s->dist));
        f4 lightColor = sc->mats[lp->matIdx].emittance;
        f4 Ld = muls(mul4(muls(lightColor, solidAngle), s->BRDF), s->dotNL);
        f4 color = firefly(mul4(Ld, s->intensity), cfg);
        accum[s->pixelIdx] = add4(accum[s->pixelIdx], color);
    }
    if (ctr) { ctr->rays += local.rays; ctr->tlas_visits += local.tlas_visits; ctr->inst_visits += local.inst_visits;
               ctr->node_visits += local.node_visits; ctr->prim_tests += local.prim_tests; }
}
/* The traversal work of orc_connect ray by ray, nothing accumulated: work[i] belongs to shadow[i] whatever the schedule, and the sums
 * over i are what orc_connect adds to its counters for the same queue and config (connect_order included). */
void orc_connect_work(const RtShadowRay* shadow, int32_t n, const OrcScene* sc, const OrcConfig* cfg, OrcRayWork* work)
{
    for (int32_t i = 0; i < n; i++) {
        const RtShadowRay* s = &shadow[i];
        OrcCounters c; memset(&c, 0, sizeof c);
        RtRay ray = zero_ray();
        init_ray(&ray, add4(s->I, muls(s->L, RT_EPSILON)), s->L);
        ray.t = s->dist - 2 * RT_EPSILON;
        const int occluded = traverse_tlas(&ray, sc, cfg, 1, &c) == -1;
        work[i].node_visits = (uint32_t)c.node_visits; work[i].prim_tests = (uint32_t)c.prim_tests;
        work[i].tlas_visits = (uint32_t)c.tlas_visits; work[i].inst_visits = (uint32_t)c.inst_visits;
        work[i].occluded = (uint32_t)occluded;
    }
}
/* orc_connect's traversal on rays given as they are traced: origin[i], dir[i] (xyz; the w lanes are taken as 0) with reach tmax[i]
 * (NULL: RT_REALLYFAR).  occluded[i] = 1 iff a primitive is accepted with t < tmax[i].  A record {I, L, dist} of orc_connect is the ray
 * I + L * eps, L with tmax = dist - 2 eps. */
void orc_occluded(const RtFloat4* origin, const RtFloat4* dir, const float* tmax, int32_t n, const OrcScene* sc, const OrcConfig* cfg, uint8_t* occluded)
{
    for (int32_t i = 0; i < n; i++) {
        OrcCounters c; memset(&c, 0, sizeof c);
        RtRay ray = zero_ray();
        init_ray(&ray, v4(origin[i].x, origin[i].y, origin[i].z, 0.0f), v4(dir[i].x, dir[i].y, dir[i].z, 0.0f));
        ray.t = tmax ? tmax[i] : RT_REALLYFAR;
        occluded[i] = traverse_tlas(&ray, sc, cfg, 1, &c) == -1;
    }
}
float orc_focus(int32_t x, int32_t y, const OrcScene* sc, const OrcConfig* cfg, const RtCamera* cam) /* wavefront.cl:203-224 */
{
    RtRay r = zero_ray(); OrcCounters c; memset(&c, 0, sizeof c);
    primary_ray_simple(&r, x, y, cam, cfg->width, cfg->height);
    traverse_tlas(&r, sc, cfg, 0, &c);
    return r.t;
}

/* ---------------------------------------------------------------- frame driver (renderer.cpp:64-94) */
size_t orc_frame_work_bytes(int32_t n, const OrcConfig* cfg)
{
    return (size_t)n * (2 * sizeof(RtRay) + (size_t)(cfg->max_bounces > 0 ? cfg->max_bounces : 1) * sizeof(RtShadowRay));
}
void orc_render_frame(const OrcScene* sc, const OrcConfig* cfg, const RtCamera* cam, int32_t aa,
                      int32_t firstPixel, int32_t n, RtFloat4* accum, uint32_t* seeds, void* work,
                      OrcCounters* extendCtr, OrcCounters* connectCtr)
{
    RtRay* ray1 = (RtRay*)work;
    RtRay* ray2 = ray1 + n;
    RtShadowRay* shadow = (RtShadowRay*)(ray2 + n);
    int32_t nIn = n, nShadow = 0;
    orc_generate(ray1, n, firstPixel, cfg, cam, aa, seeds);
    for (int b = 0; b < cfg->max_bounces; b++) {
        orc_extend(ray1, nIn, sc, cfg, 0, NULL, NULL, extendCtr);
        int32_t nOut = 0;
        orc_shade(ray1, nIn, ray2, &nOut, shadow, &nShadow, sc, cfg, accum, seeds);
        if (!cfg->russian_roulette && cfg->shading == ORC_SHADING_NEE) { /* renderer.cpp:85-87 */
            orc_connect(shadow, nShadow, sc, cfg, accum, connectCtr);
            nShadow = 0;                                                  /* wavefront.cl:54-56 */
        }
        RtRay* t = ray1; ray1 = ray2; ray2 = t;
        nIn = nOut;
    }
    if (cfg->russian_roulette) orc_connect(shadow, nShadow, sc, cfg, accum, connectCtr); /* renderer.cpp:91-92 */
}

static void add_ctr(OrcCounters* d, const OrcCounters* s)
{
    if (!d) return;
    d->rays += s->rays; d->tlas_visits += s->tlas_visits; d->inst_visits += s->inst_visits;
    d->node_visits += s->node_visits; d->prim_tests += s->prim_tests;
}
void orc_render_bands(const OrcScene* sc, const OrcConfig* cfg, const RtCamera* cam, int32_t aa,
                      int32_t y0, int32_t y1, int32_t frames, int32_t threads, RtFloat4* accum, uint32_t* seeds,
                      OrcCounters* extendCtr, OrcCounters* connectCtr)
{
    if (threads < 1) threads = 1;
    int rows = y1 - y0;
    if (threads > rows) threads = rows;
#pragma omp parallel for num_threads(threads) schedule(static, 1)
    for (int b = 0; b < threads; b++) {
        int r0 = y0 + (int)((int64_t)rows * b / threads), r1 = y0 + (int)((int64_t)rows * (b + 1) / threads);
        int32_t first = r0 * cfg->width, n = (r1 - r0) * cfg->width;
        void* work = malloc(orc_frame_work_bytes(n, cfg));
        OrcCounters e, c; memset(&e, 0, sizeof e); memset(&c, 0, sizeof c);
        for (int f = 0; f < frames; f++)
            orc_render_frame(sc, cfg, cam, aa, first, n, accum, seeds + (first - y0 * cfg->width), work, &e, &c);
        free(work);
#pragma omp critical
        { add_ctr(extendCtr, &e); add_ctr(connectCtr, &c); }
    }
}
void orc_trace_normals(const OrcScene* sc, const OrcConfig* cfg, const RtCamera* cam, int32_t threads, RtFloat4* out)
{
    if (threads < 1) threads = 1;
#pragma omp parallel for num_threads(threads) schedule(dynamic, 4)
    for (int y = 0; y < cfg->height; y++) {
        OrcCounters c; memset(&c, 0, sizeof c);
        for (int x = 0; x < cfg->width; x++) {
            RtRay r = zero_ray();
            primary_ray_simple(&r, x, y, cam, cfg->width, cfg->height);
            traverse_tlas(&r, sc, cfg, 0, &c);
            finish_hit(&r, sc);
            out[y * cfg->width + x] = r.primIdx == -1 ? splat(0.0f)
                : muls(add4(r.N, splat(1.0f)), 0.5f);
        }
    }
}

/* ---------------------------------------------------------------- post-processing (src/cl/postproc.cl, renderer.cpp:95-124) */
static void post_chain(const RtFloat4* accum, int idx, int W, int H, float invFrames, float vignette, float gamma, float out[3])
{
    float c[3] = { fminf(accum[idx].x * invFrames, 1.0f), fminf(accum[idx].y * invFrames, 1.0f), fminf(accum[idx].z * invFrames, 1.0f) }; /* prep :65-75 */
    if (vignette > 0) { /* vignetting :18-32; length/smoothstep/mix as in ROCm's OpenCL library */
        int x = idx % W, y = idx / W;
        float px = (float)x / (float)W - 0.5f, py = (float)y / (float)H - 0.5f;
        float d = fmaf(py, py, px * px);
        float len = d < FLT_MIN ? sqrtf(fmaf(py * 0x1p+86f, py * 0x1p+86f, (px * 0x1p+86f) * (px * 0x1p+86f))) * 0x1p-86f : sqrtf(d);
        float t = fminf(fmaxf(len, 0.0f), 1.0f);
        float vig = 1 - (t * t) * fmaf(t, -2.0f, 3.0f);
        for (int k = 0; k < 3; k++) c[k] = fmaf(c[k] * vig - c[k], vignette, c[k]);
    }
    if (gamma != 1.0f) for (int k = 0; k < 3; k++) c[k] = powf(c[k], gamma); /* gammaCorr :34-40 */
    out[0] = c[0]; out[1] = c[1]; out[2] = c[2];
}
void orc_postproc(const RtFloat4* accum, int32_t W, int32_t H, int32_t frames, float vignette, float gamma, float chromatic,
                  RtFloat4* outF, uint8_t* outRGBA8)
{
    float inv = 1 / (float)frames;
    for (int idx = 0; idx < W * H; idx++) {
        float c[3], p[3];
        post_chain(accum, idx, W, H, inv, vignette, gamma, c);
        if (chromatic > 0 && idx % W != 0) { /* chromatic :42-63 */
            post_chain(accum, idx - 1, W, H, inv, vignette, gamma, p);
            float o = chromatic;
            c[1] = c[1] * (1 - o) + p[1] * o;
            c[2] = c[2] * (1 - 2 * o) + p[2] * 2 * o;
        }
        float r = fminf(c[0], 1.0f), g = fminf(c[1], 1.0f), b = fminf(c[2], 1.0f); /* saveImage :77-86 */
        if (outF) outF[idx] = v4(r, g, b, 1.0f);
        if (outRGBA8) { outRGBA8[4 * idx] = (uint8_t)(r * 255); outRGBA8[4 * idx + 1] = (uint8_t)(g * 255); outRGBA8[4 * idx + 2] = (uint8_t)(b * 255); outRGBA8[4 * idx + 3] = 255; }
    }
}

/* ---------------------------------------------------------------- unit hooks for the known-answer tests */
void orc_test_random_float3(uint32_t* seed, float out[4]) { f4 r = rnd_float3(seed); out[0] = r.x; out[1] = r.y; out[2] = r.z; out[3] = r.w; }
void orc_test_cosine_hemisphere(const float N[4], uint32_t* seed, float out[4])
{
    f4 r = cosine_ray_hemisphere(v4(N[0], N[1], N[2], N[3]), seed);
    out[0] = r.x; out[1] = r.y; out[2] = r.z; out[3] = r.w;
}
void orc_test_triangle(const float v0[3], const float v1[3], const float v2[3], const float O[3], const float D[3], float out[4])
{
    RtTriangle t; memset(&t, 0, sizeof t);
    t.v0 = v4(v0[0], v0[1], v0[2], 0); t.v1 = v4(v1[0], v1[1], v1[2], 0); t.v2 = v4(v2[0], v2[1], v2[2], 0);
    RtRay r = zero_ray(); init_ray(&r, v4(O[0], O[1], O[2], 0), v4(D[0], D[1], D[2], 0));
    isect_triangle(7, &t, &r);
    out[0] = r.t; out[1] = r.u; out[2] = r.v; out[3] = (float)r.primIdx;
}
uint32_t orc_test_wang_hash(uint32_t s) /* util.cl:37-44 (unused on the path; known answer WangHash(1)) */
{
    s = (s ^ 61) ^ (s >> 16); s *= 9; s = s ^ (s >> 4); s *= 0x27d4eb2d; s = s ^ (s >> 15);
    return s;
}

/* ---------------------------------------------------------------- the math functions on their own (oracle.h, RT_MATH_*) */
static inline uint32_t f32_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static uint32_t math_one(int fn, uint32_t bits)
{
    float x = bits_f32(bits);
    switch (fn) {
    case RT_MATH_EXP: return f32_bits(orc_expf(x));
    case RT_MATH_SIN: return f32_bits(orc_sinf(x));
    case RT_MATH_COS: return f32_bits(orc_cosf(x));
    case RT_MATH_ACOS: return f32_bits(orc_acosf(x));
    case RT_MATH_ATAN: return f32_bits(orc_atan2f(x, 1.0f));
    case RT_MATH_F2I: return (uint32_t)f2i_gpu(x);
    }
    return 0;
}
int orc_math(int32_t fn, const void* in, void* out, int64_t n)
{
    if (fn < RT_MATH_EXP || fn > RT_MATH_LENGTH4 || n < 0) return -1;
    const uint32_t* a = (const uint32_t*)in;
    uint32_t* o = (uint32_t*)out;
    for (int64_t i = 0; i < n; i++) {
        switch (fn) {
        case RT_MATH_ATAN2: o[i] = f32_bits(orc_atan2f(bits_f32(a[2 * i]), bits_f32(a[2 * i + 1]))); break;
        case RT_MATH_SPHERE_TEXEL: {
            const uint32_t* e = a + 6 * i;
            int x, y;
            orc_sphere_texel_xy(v4(bits_f32(e[0]), bits_f32(e[1]), bits_f32(e[2]), bits_f32(e[3])), (int)e[4], (int)e[5], &x, &y);
            o[2 * i] = (uint32_t)x; o[2 * i + 1] = (uint32_t)y;
        } break;
        case RT_MATH_NORMALIZE4:
        case RT_MATH_LENGTH4: {
            const uint32_t* e = a + 4 * i;
            f4 v = v4(bits_f32(e[0]), bits_f32(e[1]), bits_f32(e[2]), bits_f32(e[3]));
            if (fn == RT_MATH_LENGTH4) { o[i] = f32_bits(length4(v)); break; }
            f4 r = normalize4(v);
            o[4 * i] = f32_bits(r.x); o[4 * i + 1] = f32_bits(r.y); o[4 * i + 2] = f32_bits(r.z); o[4 * i + 3] = f32_bits(r.w);
        } break;
        default: o[i] = math_one(fn, a[i]); break;
        }
    }
    return 0;
}
static inline uint64_t splitmix64(uint64_t z)
{
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
static inline int clamp_threads(int32_t t) { return t < 1 ? 1 : (t > 16 ? 16 : t); }
int orc_math_sweep(int32_t fn, int32_t firstBlock, int32_t nBlocks, uint64_t* hashes, int32_t threads)
{
    if (fn < RT_MATH_EXP || fn > RT_MATH_F2I || firstBlock < 0 || nBlocks < 0 || firstBlock + nBlocks > (1 << (32 - RT_MATH_SWEEP_BLOCK_BITS)))
        return -1;
    #pragma omp parallel for schedule(dynamic, 1) num_threads(clamp_threads(threads))
    for (int32_t b = 0; b < nBlocks; b++) {
        uint64_t h = 0;
        const uint32_t base = (uint32_t)(firstBlock + b) << RT_MATH_SWEEP_BLOCK_BITS;
        for (uint32_t k = 0; k < (1u << RT_MATH_SWEEP_BLOCK_BITS); k++) {
            uint32_t bits = base + k, r = math_one(fn, bits);
            if (fn != RT_MATH_F2I && (r & 0x7fffffffu) > 0x7f800000u) r = 0x7fc00000u;
            h += splitmix64((uint64_t)bits << 32 | r);
        }
        hashes[b] = h;
    }
    return 0;
}
/* float spacing at a real value t (subnormal spacing below FLT_MIN) */
static inline double ulp_at(double t)
{
    int e;
    t = fabs(t);
    if (t < FLT_MIN) return 0x1p-149;
    frexp(t, &e);                    /* t in [2^(e-1), 2^e) */
    return ldexp(1.0, e - 24);
}
static double math_exact(int fn, double x)
{
    switch (fn) {
    case RT_MATH_EXP: return exp(x);
    case RT_MATH_SIN: return sin(x);
    case RT_MATH_COS: return cos(x);
    case RT_MATH_ACOS: return acos(x);
    case RT_MATH_ATAN: return atan(x);
    }
    return NAN;
}
static inline uint32_t ord_key(float f) { uint32_t u = f32_bits(f); return (u & 0x80000000u) ? ~u : u | 0x80000000u; }
static inline float ord_float(uint32_t k) { return bits_f32((k & 0x80000000u) ? k & 0x7fffffffu : ~k); }
int orc_math_error(int32_t fn, float lo, float hi, int32_t absolute, double bound, int32_t threads, OrcMathError* out)
{
    if (fn < RT_MATH_EXP || fn > RT_MATH_ATAN || !(lo <= hi) || !out) return -1;
    const uint32_t k0 = ord_key(lo), k1 = ord_key(hi);
    OrcMathError r = { 0.0, lo, 0, 0 };
    #pragma omp parallel num_threads(clamp_threads(threads))
    {
        OrcMathError m = { 0.0, lo, 0, 0 };
        #pragma omp for schedule(dynamic, 1)
        for (int64_t c = (int64_t)(k0 >> 16); c <= (int64_t)(k1 >> 16); c++) {
            uint32_t a = (uint32_t)c << 16, b = a | 0xffffu;
            if (a < k0) a = k0;
            if (b > k1) b = k1;
            for (uint64_t k = a; k <= b; k++) {
                const float x = ord_float((uint32_t)k);
                const float f = bits_f32(math_one(fn, f32_bits(x)));
                const double t = math_exact(fn, (double)x);
                double err = fabs((double)f - t);
                if (f != f) err = INFINITY;
                else if (isinf(f)) err = (float)t == f ? 0.0 : INFINITY;   /* overflow is right when the exact value rounds to it */
                err = absolute ? err * 0x1p24 : err / ulp_at(t);
                m.count++;
                if (err > bound) m.above++;
                if (err > m.max_err || (err == m.max_err && fabsf(x) < fabsf(m.arg))) { m.max_err = err; m.arg = x; }
            }
        }
        #pragma omp critical
        {
            r.count += m.count; r.above += m.above;
            if (m.max_err > r.max_err || (m.max_err == r.max_err && fabsf(m.arg) < fabsf(r.arg))) { r.max_err = m.max_err; r.arg = m.arg; }
        }
    }
    *out = r;
    return 0;
}

/* ---------------------------------------------------------------- the RNG as a linear map, and sample_ball's rejection loop over its whole cycle */
/* xorshift32 is linear over GF(2): column b of the 32x32 matrix is the image of state 1 << b. */
static void xs_matrix(uint32_t col[32]) { for (int b = 0; b < 32; b++) { uint32_t s = 1u << b; orc_xorshift32(&s); col[b] = s; } }
static inline uint32_t xs_apply(const uint32_t col[32], uint32_t s) { uint32_t r = 0; for (int b = 0; b < 32; b++) if (s >> b & 1) r ^= col[b]; return r; }
static void xs_power(uint32_t out[32], uint64_t e)   /* the matrix of e steps, by squaring */
{
    uint32_t sq[32], t[32];
    xs_matrix(sq);
    for (int b = 0; b < 32; b++) out[b] = 1u << b;
    for (; e; e >>= 1) {
        if (e & 1) { for (int b = 0; b < 32; b++) t[b] = xs_apply(sq, out[b]); memcpy(out, t, sizeof t); }
        for (int b = 0; b < 32; b++) t[b] = xs_apply(sq, sq[b]);
        memcpy(sq, t, sizeof t);
    }
}
uint32_t orc_xorshift32_jump(uint32_t state, uint64_t steps) { uint32_t m[32]; xs_power(m, steps); return xs_apply(m, state); }

/* one coordinate of sample_ball's candidate, from one draw: rnd_float * 2 - 1 (ray.cl:49 / :62) */
static inline float ball_coord(uint32_t u) { return (float)u * 2.3283064365387e-10f * 2.0f - 1.0f; }

static inline uint32_t xs_step(uint32_t x) { x ^= x << 13; x ^= x >> 17; x ^= x << 5; return x; }   /* orc_xorshift32, inlined */

enum { REJ_SEGMENTS = 4096 };
typedef struct RejRun { uint32_t len, state, index; } RejRun;   /* rejected attempts in a row; the state and attempt index the run starts from */
typedef struct RejSeg {                 /* one residue (attempt index mod 3) of one segment of the cycle */
    RejRun head, tail, best;            /* the run before the first accepted attempt; after the last; the longest between two accepted ones */
    int32_t accepted;                   /* some attempt of the residue was accepted (else head = tail = all of them) */
} RejSeg;

static void rej_count(OrcRejection* o, RejRun r)   /* a whole run: the longest so far, the first met from state 1 among equals */
{
    if (r.len > o->longest || (r.len == o->longest && r.len && r.index < o->index)) { o->longest = r.len; o->state = r.state; o->index = r.index; }
}

int orc_rejection_cycle(int32_t threads, OrcRejection* out)
{
    if (!out) return -1;
    /* Attempt i starts from state s_i (s_0 = 1) and consumes draws s_{i+1}, s_{i+2}, s_{i+3}; the attempt that follows a rejected
     * attempt i is i + 3.  The period 2^32 - 1 is a multiple of 3, so the three residues close on themselves. */
    const uint64_t P = 0xffffffffull;
    const uint64_t L = (P / REJ_SEGMENTS / 3 + 1) * 3;
    const int S = (int)((P + L - 1) / L);
    uint32_t* start = (uint32_t*)malloc(sizeof(uint32_t) * (size_t)(2 * S + 1));
    RejSeg* seg = (RejSeg*)calloc((size_t)S * 3, sizeof(RejSeg));
    uint64_t* rejected = (uint64_t*)calloc((size_t)S, sizeof(uint64_t));
    if (!start || !seg || !rejected) { free(start); free(seg); free(rejected); return -1; }
    uint32_t* end = start + S + 1;
    uint32_t jump[32];
    xs_power(jump, L);
    start[0] = 1;
    for (int s = 0; s < S; s++) start[s + 1] = xs_apply(jump, start[s]);
    #pragma omp parallel for schedule(dynamic, 8) num_threads(clamp_threads(threads))
    for (int s = 0; s < S; s++) {
        const uint64_t first = (uint64_t)s * L, n = first + L <= P ? L : P - first;
        RejSeg* r = &seg[3 * s];
        RejRun run[3];
        memset(run, 0, sizeof run);
        uint32_t prev = start[s], a = xs_step(prev), b = xs_step(a), c = xs_step(b);
        float x = ball_coord(a), y = ball_coord(b), z = ball_coord(c);
        uint64_t rej = 0;
        int k = 0;
        for (uint64_t i = 0; i < n; i++) {
            if (x * x + y * y + z * z > 1.0f) {
                if (run[k].len++ == 0) { run[k].state = prev; run[k].index = (uint32_t)(first + i); }
                rej++;
            } else {
                if (!r[k].accepted) { r[k].accepted = 1; r[k].head = run[k]; }
                else if (run[k].len > r[k].best.len) r[k].best = run[k];
                run[k].len = 0;
            }
            prev = a; a = b; b = c; c = xs_step(c);
            x = y; y = z; z = ball_coord(c);
            k = k == 2 ? 0 : k + 1;
        }
        for (k = 0; k < 3; k++) {
            r[k].tail = run[k];
            if (!r[k].accepted) r[k].head = run[k];
        }
        rejected[s] = rej;
        end[s] = prev;
    }
    OrcRejection o;
    memset(&o, 0, sizeof o);
    o.states = P;
    o.closed = 1;
    for (int s = 0; s < S; s++) {           /* the walks join up (which checks the jump-ahead too) and return to state 1 after 2^32 - 1 steps */
        if (end[s] != (s + 1 < S ? start[s + 1] : 1u)) o.closed = 0;
        o.rejected += rejected[s];
    }
    for (int k = 0; k < 3; k++) {
        RejRun carry = { 0, 0, 0 };
        int open = 0;                       /* a run is being carried (it may have length 0: an accepted attempt ended the segment) */
        for (int s = 0; s < 2 * S; s++) {   /* second lap: the run open at the end of the cycle joins the first segments' */
            const RejSeg* g = &seg[3 * (s % S) + k];
            if (s >= S && !open) break;
            if (s < S) rej_count(&o, g->best);
            RejRun joined = carry.len ? carry : g->head;
            joined.len = carry.len + g->head.len;
            if (!g->accepted) { carry = joined; continue; }   /* no accepted attempt in the whole segment */
            if (open) rej_count(&o, joined);     /* (the run before the cycle's first accepted attempt waits for the second lap) */
            if (s >= S) break;
            carry = g->tail; open = 1;
        }
    }
    free(start); free(seg); free(rejected);
    *out = o;
    return 0;
}

// rt355_math.h — the kernels' arithmetic as one unit: the float4 helpers, the two arithmetics (RT_BUILTINS_IEEE / RT_BUILTINS_REFERENCE)
// with their transcendentals, the float -> int rule and the sphere texel lookup built on them.  This is what rt_debug_math probes
// (math_debug.hip) and tests/mathsets.py pins; rt355_kernels.h includes it for the renderer.  Nothing here emits code on its own.
#pragma once
#include "rt355_dev.h"
#include "../../include/rt355.h"

namespace rt355dev {

// ------------------------------------------------------------------ float4 helpers
// Non-temporal accesses for queue data at its LAST use (k_shade's input entries and hit records, k_accumulate's shadow records) and for
// k_generate's primary rays: what streams through once does not push node and triangle records out of the L2s.  Measured with the
// accesses switched one group at a time (profiles/r02_nt_streams.txt): +1.0 % with three lanes, +1.4 % for one context; the same hint on
// k_shade's STORES costs a context alone 1 % (the next extend reads them back soon), on the traversal kernels' ray loads and hit stores nothing.
typedef float nt_v4f __attribute__((ext_vector_type(4)));
typedef unsigned nt_v2u __attribute__((ext_vector_type(2)));
RT_FORCEINLINE float4 ldnt4(const float4* p) { nt_v4f t = __builtin_nontemporal_load((const nt_v4f*)p); return *(float4*)&t; }
RT_FORCEINLINE uint2 ldnt2(const uint2* p) { nt_v2u t = __builtin_nontemporal_load((const nt_v2u*)p); return *(uint2*)&t; }
RT_FORCEINLINE void stnt4(float4* p, float4 v) { __builtin_nontemporal_store(*(nt_v4f*)&v, (nt_v4f*)p); }
RT_FORCEINLINE void stnt2(uint2* p, uint2 v) { __builtin_nontemporal_store(*(nt_v2u*)&v, (nt_v2u*)p); }
RT_FORCEINLINE float4 mk4(float x, float y, float z, float w) { return make_float4(x, y, z, w); }
RT_FORCEINLINE float4 splat(float s) { return make_float4(s, s, s, s); }
RT_FORCEINLINE float4 add4(float4 a, float4 b) { return mk4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
RT_FORCEINLINE float4 sub4(float4 a, float4 b) { return mk4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
RT_FORCEINLINE float4 mul4(float4 a, float4 b) { return mk4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
RT_FORCEINLINE float4 muls(float4 a, float s) { return mk4(a.x * s, a.y * s, a.z * s, a.w * s); }
RT_FORCEINLINE float4 neg4(float4 a) { return mk4(-a.x, -a.y, -a.z, -a.w); }
RT_FORCEINLINE float4 ld4(const RtFloat4& v) { return *reinterpret_cast<const float4*>(&v); }
RT_FORCEINLINE float dot3(float4 a, float4 b) { return __fmaf_rn(a.z, b.z, __fmaf_rn(a.y, b.y, a.x * b.x)); }
RT_FORCEINLINE float dot4(float4 a, float4 b) { return __fmaf_rn(a.w, b.w, __fmaf_rn(a.z, b.z, __fmaf_rn(a.y, b.y, a.x * b.x))); }
RT_FORCEINLINE float4 cross4(float4 a, float4 b)
{
    return mk4(__fmaf_rn(a.y, b.z, b.y * (-a.z)), __fmaf_rn(a.z, b.x, b.z * (-a.x)), __fmaf_rn(a.x, b.y, b.x * (-a.y)), 0.0f);
}
// Two arithmetics, chosen per context (RtConfig.builtins) and carried down to here as the template parameter REFB of every function
// that reaches one of the seven builtins; each kernel that does exists in both instantiations, and the host picks one per launch.
// REFB = false (RT_BUILTINS_IEEE, the default): IEEE 1/sqrt and the Cephes sequences, what a CPU (the oracle) reproduces bit for bit.
// REFB = true (RT_BUILTINS_REFERENCE; what RT_BUILTINS_DEFAULT means in librt355_refb.so, -DRT355_REF_BUILTINS): the builtins evaluate the
// very instruction sequences ROCm's OpenCL library gives the reference's kernels - normalize() = v * rsqrt(dot) with the hardware
// v_rsq_f32 (opencl.bc _Z9normalizeDv4_f -> __ocml_rsqrt_f32), length() = the hardware v_sqrt_f32 (llvm.sqrt with !fpmath 3 ulp in
// _Z6lengthDv4_f), exp / sin / cos / acospi / atan2pi = the same ocml bitcode functions the OpenCL builtins resolve to (HIP links the same
// ocml.bc with the same control constants: correctly rounded sqrt on, denormals on, no unsafe math).  With them the HIP path is held to
// the reference's own kernels WITHOUT the few-ulp allowance of DESIGN.md section 2, on uncurated frames (tests/test_gpu_builtins.py).
extern "C" __device__ float __ocml_acospi_f32(float);
extern "C" __device__ float __ocml_atan2pi_f32(float, float);
// RT_BUILTINS_DEFAULT is IEEE in the shipped library; -DRT355_REF_BUILTINS (librt355_refb.so) changes that and nothing else
#ifdef RT355_REF_BUILTINS
static constexpr int32_t kDefaultBuiltins = RT_BUILTINS_REFERENCE;
#else
static constexpr int32_t kDefaultBuiltins = RT_BUILTINS_IEEE;
#endif
static bool resolve_builtins(int32_t word, int32_t* mode)
{
    if (word == RT_BUILTINS_DEFAULT) word = kDefaultBuiltins;
    if (word != RT_BUILTINS_IEEE && word != RT_BUILTINS_REFERENCE) return false;
    *mode = word;
    return true;
}
template <bool REFB> RT_FORCEINLINE float rt_len_sqrt(float d) { if constexpr (REFB) return __builtin_amdgcn_sqrtf(d); else return sqrtf(d); }
template <bool REFB> RT_FORCEINLINE float rt_rsqrt(float d) { if constexpr (REFB) return __ocml_rsqrt_f32(d); else return 1.0f / sqrtf(d); }
template <bool REFB> RT_FORCEINLINE float length4(float4 v)
{
    float d = dot4(v, v);
    if (d < 1.17549435e-38f) { float4 s = muls(v, 0x1p+86f); return rt_len_sqrt<REFB>(dot4(s, s)) * 0x1p-86f; }
    if (d == INFINITY) { float4 s = muls(v, 0x1p-66f); return rt_len_sqrt<REFB>(dot4(s, s)) * 0x1p+66f; }
    return rt_len_sqrt<REFB>(d);
}
RT_FORCEINLINE float sel_inf(float x) { return copysignf(isinf(x) ? 1.0f : 0.0f, x); }
template <bool REFB> RT_FORCEINLINE float4 normalize4(float4 v)
{
    if (v.x == 0.0f && v.y == 0.0f && v.z == 0.0f && v.w == 0.0f) return v;
    float d = dot4(v, v);
    if (d < 1.17549435e-38f) { v = muls(v, 0x1p+86f); d = dot4(v, v); }
    else if (d == INFINITY) {
        v = muls(v, 0x1p-66f); d = dot4(v, v);
        if (d == INFINITY) { v = mk4(sel_inf(v.x), sel_inf(v.y), sel_inf(v.z), sel_inf(v.w)); d = dot4(v, v); }
    }
    float r = rt_rsqrt<REFB>(d);
    return muls(v, r);
}

// ------------------------------------------------------------------ transcendentals
// exp (Beer's law, glass.cl:4-9), sin / cos (fisheye camera, sphere-light sampling), acos / atan2 (sphere texture lookup).  The
// device library's versions lean on hardware approximations (v_exp_f32, v_sin_f32 ...) that no CPU reproduces, and one last-bit
// difference in a Fresnel draw or a texel index flips a whole path; so this path and the CPU oracle both evaluate the single-precision
// Cephes algorithms (S. Moshier: expf.c, sinf.c, asinf.c, atanf.c) as plain sequences of IEEE + - * / sqrt - transcribed separately
// here and in oracle/oracle.c - and agree bit for bit on every input (tests/test_gpu_math.py).  Error against float64 (DESIGN.md section
// 2, asserted by tests/test_math_cpu.py): exp <= 1 ulp, acos <= 1.3 ulp, atan <= 2.9 ulp, atan2 <= 3.4 ulp, sin / cos <= 1.32 * 2^-24
// absolute for |x| <= 8192 (0 beyond).  These are the *_ieee functions; rt_expf / rt_sinf / rt_cosf<REFB> behind them choose between
// them and the ocml functions (REFB, see above).  acos / atan2 are called by the IEEE texel lookup only (sphere_texel_xy<false>).
RT_FORCEINLINE float rt_expf_ieee(float x)
{
    if (x != x) return x;
    if (x > 88.7228394f) return INFINITY;
    if (x < -103.972076f) return 0.0f;
    const float n = floorf(x * 1.44269504088896341f + 0.5f);
    float r = x - n * 0.693359375f;
    r = r - n * -2.12194440e-4f;
    const float z = r * r;
    float p = 1.9875691500E-4f;
    p = p * r + 1.3981999507E-3f;
    p = p * r + 8.3334519073E-3f;
    p = p * r + 4.1665795894E-2f;
    p = p * r + 1.6666665459E-1f;
    p = p * r + 5.0000001201E-1f;
    float e = p * z;
    e = e + r;
    e = e + 1.0f;
    int k = (int)n;
    if (k > 127) { e = e * 0x1p127f; k -= 127; }
    else if (k < -126) { e = e * 0x1p-126f; k += 126; }
    return e * __uint_as_float((uint32_t)(k + 127) << 23);
}
RT_FORCEINLINE float rt_trig_reduce(float ax, int& j)   // octant (made even-up) and remainder in [-pi/4, pi/4], three-term Cody-Waite
{
    j = (int)(1.27323954473516f * ax);
    float y = (float)j;
    if (j & 1) { j += 1; y = y + 1.0f; }
    j &= 7;
    float r = ax - y * 0.78515625f;
    r = r - y * 2.4187564849853515625e-4f;
    r = r - y * 3.77489497744594108e-8f;
    return r;
}
RT_FORCEINLINE float rt_sin_kernel(float x, float z) { float p = -1.9515295891E-4f * z + 8.3321608736E-3f; p = p * z - 1.6666654611E-1f; p = p * z; p = p * x; return p + x; }
RT_FORCEINLINE float rt_cos_kernel(float z) { float p = 2.443315711809948E-005f * z - 1.388731625493765E-003f; p = p * z + 4.166664568298827E-002f; p = p * z; p = p * z; p = p - 0.5f * z; return p + 1.0f; }
RT_FORCEINLINE float rt_sinf_ieee(float x)
{
    if (x != x) return x;
    bool neg = x < 0.0f;
    const float ax = neg ? -x : x;
    if (x == 0.0f) return x;   // sin(-0) = -0
    if (ax == INFINITY) return x - x;   // NaN
    if (ax > 8192.0f) return 0.0f;
    int j; const float r = rt_trig_reduce(ax, j);
    if (j > 3) { neg = !neg; j -= 4; }
    const float z = r * r;
    const float y = (j == 1 || j == 2) ? rt_cos_kernel(z) : rt_sin_kernel(r, z);
    return neg ? -y : y;
}
RT_FORCEINLINE float rt_cosf_ieee(float x)
{
    if (x != x) return x;
    const float ax = x < 0.0f ? -x : x;
    if (ax == INFINITY) return x - x;   // NaN
    if (ax > 8192.0f) return 0.0f;
    int j; const float r = rt_trig_reduce(ax, j);
    bool neg = false;
    if (j > 3) { neg = !neg; j -= 4; }
    if (j > 1) neg = !neg;
    const float z = r * r;
    const float y = (j == 1 || j == 2) ? rt_sin_kernel(r, z) : rt_cos_kernel(z);
    return neg ? -y : y;
}
RT_FORCEINLINE float rt_asinf(float x)
{
    const bool neg = x < 0.0f;
    const float a = neg ? -x : x;
    if (a > 1.0f) return (x - x) / (x - x);
    if (a < 1.0e-4f) return x;
    float z, w; bool flag = false;
    if (a > 0.5f) { z = 0.5f * (1.0f - a); w = sqrtf(z); flag = true; }
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
RT_FORCEINLINE float rt_acosf(float x)
{
    if (x != x) return x;
    if (x < -1.0f || x > 1.0f) return (x - x) / (x - x);   // NaN: a non-unit sphere normal (w-lane pollution) gets here; f2i_gpu then reads texel row 0
    if (x < -0.5f) return 3.14159265358979323846f - 2.0f * rt_asinf(sqrtf(0.5f * (1.0f + x)));
    if (x > 0.5f) return 2.0f * rt_asinf(sqrtf(0.5f * (1.0f - x)));
    return 1.5707963267948966192f - rt_asinf(x);
}
RT_FORCEINLINE float rt_atanf(float x)
{
    const bool neg = signbit(x);   // atan(-0) = -0
    float a = neg ? -x : x, y;
    if (a > 2.414213562373095f) { y = 1.5707963267948966192f; a = -(1.0f / a); }
    else if (a > 0.4142135623730950f) { y = 0.7853981633974483096f; a = (a - 1.0f) / (a + 1.0f); }
    else y = 0.0f;
    const float z = a * a;
    float p = 8.05374449538e-2f * z - 1.38776856032E-1f;
    p = p * z + 1.99777106478E-1f;
    p = p * z - 3.33329491539E-1f;
    p = p * z;
    p = p * a;
    p = p + a;
    y = y + p;
    return neg ? -y : y;
}
RT_FORCEINLINE float rt_atan2f(float y, float x)
{
    if (x != x || y != y) return x + y;
    if (x == 0.0f) {
        if (y == 0.0f) return signbit(x) ? copysignf(3.14159265358979323846f, y) : y;
        return y > 0.0f ? 1.5707963267948966192f : -1.5707963267948966192f;
    }
    if (isinf(x) && isinf(y)) return copysignf(x > 0.0f ? 0.7853981633974483096f : 2.3561944901923449288f, y);
    float z = rt_atanf(y / x);
    if (x < 0.0f) z = signbit(y) ? z - 3.14159265358979323846f : z + 3.14159265358979323846f;
    return z;
}
template <bool REFB> RT_FORCEINLINE float rt_expf(float x) { if constexpr (REFB) return __ocml_exp_f32(x); else return rt_expf_ieee(x); }
template <bool REFB> RT_FORCEINLINE float rt_sinf(float x) { if constexpr (REFB) return __ocml_sin_f32(x); else return rt_sinf_ieee(x); }
template <bool REFB> RT_FORCEINLINE float rt_cosf(float x) { if constexpr (REFB) return __ocml_cos_f32(x); else return rt_cosf_ieee(x); }

// float -> int with the hardware's own rule (v_cvt_i32_f32 / v_cvt_u32_f32: NaN -> 0, out of range saturates), spelled out so that it
// is defined C++ rather than a poison fptosi.  It matters: a sphere hit found with w-lane-polluted dots has a non-unit normal,
// acos(N.y) is then NaN and the reference's kernels read texel row 0 (tests/test_gpu_reference.py, whole-frame comparison).
RT_FORCEINLINE int f2i_gpu(float x) { return x != x ? 0 : (x >= 2147483648.0f ? 2147483647 : (x <= -2147483648.0f ? (int)(-2147483647 - 1) : (int)x)); }
// Texel column / row of a sphere hit with normal N (primitives.cl:130-133).  The seam N.z = +-0, N.x < 0 gives ux = 1 or 0 by the
// sign of N.z, and the pole N.y = -1 gives uy = 1: x = texW and y = texH are the reference's indices there (tests/test_gpu_math.py).
template <bool REFB> RT_FORCEINLINE void sphere_texel_xy(float4 N, int texW, int texH, int& x, int& y)
{
    float ux, uy;
    if constexpr (REFB) {
        ux = (1.0f + __ocml_atan2pi_f32(N.z, N.x)) * 0.5f;   // primitives.cl:130 (int + float is a float add; * 0.5 is exact in any precision)
        uy = __ocml_acospi_f32(N.y);                         // :131
    } else {
        ux = (float)((1 + rt_atan2f(N.z, N.x) / 3.14159265358979323846) * 0.5);
        uy = rt_acosf(N.y) / 3.14159265358979323846f;
    }
    x = f2i_gpu(ux * (float)texW);
    y = f2i_gpu(uy * (float)texH);
}

} // namespace rt355dev

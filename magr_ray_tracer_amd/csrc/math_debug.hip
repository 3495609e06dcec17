// math_debug.hip — the kernels' math functions on their own (rt_debug_math*, include/rt355.h; tests/test_gpu_math.py,
// tests/test_gpu_builtins.py).  No context and no scene: the functions of rt355_math.h, which the renderer's kernels call, evaluated over
// the caller's inputs on device 0.  Each case calls the function the renderer calls; nothing here restates one.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "rt355_dev.h"
#include "rt355_math.h"
#include "scene_dev.h"   // fail, HIPCHK

using namespace rt355dev;

// REFB as in rt355_math.h; the REFERENCE set has no acos / atan of its own (it calls acospi / atan2pi inside the texel lookup only).
template <bool REFB> static __device__ __forceinline__ uint32_t math_one(int fn, uint32_t bits)
{
    const float x = __uint_as_float(bits);
    float r;
    switch (fn) {
    case RT_MATH_EXP: r = rt_expf<REFB>(x); break;
    case RT_MATH_SIN: r = rt_sinf<REFB>(x); break;
    case RT_MATH_COS: r = rt_cosf<REFB>(x); break;
    case RT_MATH_F2I: return (uint32_t)f2i_gpu(x);
    case RT_MATH_ACOS: if constexpr (!REFB) { r = rt_acosf(x); break; }   // REFB: not a function of that set (the host refuses it)
    case RT_MATH_ATAN: if constexpr (!REFB) { r = rt_atan2f(x, 1.0f); break; }
    default: r = 0.0f; break;
    }
    return __float_as_uint(r);
}
template <bool REFB>
__global__ __launch_bounds__(kBlock) void k_debug_math(int fn, const uint32_t* in, uint32_t* out, int64_t n)
{
    for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const uint32_t* a = in;
        uint32_t* o = out;
        switch (fn) {
        case RT_MATH_SPHERE_TEXEL: {
            const uint32_t* e = a + 6 * i;
            const float4 N = mk4(__uint_as_float(e[0]), __uint_as_float(e[1]), __uint_as_float(e[2]), __uint_as_float(e[3]));
            int x, y;
            sphere_texel_xy<REFB>(N, (int)e[4], (int)e[5], x, y);
            o[2 * i] = (uint32_t)x; o[2 * i + 1] = (uint32_t)y;
        } break;
        case RT_MATH_NORMALIZE4:
        case RT_MATH_LENGTH4: {
            const uint32_t* e = a + 4 * i;
            const float4 v = mk4(__uint_as_float(e[0]), __uint_as_float(e[1]), __uint_as_float(e[2]), __uint_as_float(e[3]));
            if (fn == RT_MATH_LENGTH4) { o[i] = __float_as_uint(length4<REFB>(v)); break; }
            const float4 r = normalize4<REFB>(v);
            o[4 * i] = __float_as_uint(r.x); o[4 * i + 1] = __float_as_uint(r.y); o[4 * i + 2] = __float_as_uint(r.z); o[4 * i + 3] = __float_as_uint(r.w);
        } break;
        case RT_MATH_ATAN2: if constexpr (!REFB) { o[i] = __float_as_uint(rt_atan2f(__uint_as_float(a[2 * i]), __uint_as_float(a[2 * i + 1]))); break; }   // REFB: as in math_one
        default: o[i] = math_one<REFB>(fn, a[i]); break;
        }
    }
}
static constexpr int kSweepPerThread = 64;   // a workgroup hashes 256 x 64 = 2^14 inputs; a block of 2^20 takes 64 workgroups
template <bool REFB>
__global__ __launch_bounds__(kBlock) void k_debug_math_sweep(int fn, uint32_t firstBlock, unsigned long long* hashes)
{
    __shared__ unsigned long long part[kBlock];
    constexpr uint32_t perGroup = kBlock * kSweepPerThread, groupsPerBlock = (1u << RT_MATH_SWEEP_BLOCK_BITS) / perGroup;
    const uint32_t blk = blockIdx.x / groupsPerBlock;
    const uint32_t base = ((firstBlock + blk) << RT_MATH_SWEEP_BLOCK_BITS) + (blockIdx.x % groupsPerBlock) * perGroup;
    unsigned long long h = 0;
    for (int k = 0; k < kSweepPerThread; k++) {
        const uint32_t bits = base + (uint32_t)k * kBlock + threadIdx.x;
        uint32_t r = math_one<REFB>(fn, bits);
        if (fn != RT_MATH_F2I && (r & 0x7fffffffu) > 0x7f800000u) r = 0x7fc00000u;
        unsigned long long z = ((unsigned long long)bits << 32 | r) + 0x9e3779b97f4a7c15ull;   // splitmix64
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        h += z ^ (z >> 31);
    }
    part[threadIdx.x] = h;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicAdd(&hashes[blk], part[0]);
}
static int math_device(const char* who)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(RT_E_DEVICE, "%s: no HIP device visible (this library has no CPU path)", who);
    HIPCHK(hipSetDevice(0));
    return RT_OK;
}
extern "C" int rt_debug_math_mode(int32_t builtins, int32_t fn, const void* in, void* out, int64_t n)
{
    int32_t mode;
    if (!resolve_builtins(builtins, &mode)) return fail(RT_E_INVALID, "rt_debug_math: builtins = %d is none of RT_BUILTINS_DEFAULT (0), RT_BUILTINS_IEEE (1), RT_BUILTINS_REFERENCE (2)", builtins);
    const bool refb = mode == RT_BUILTINS_REFERENCE;
    static const int inWords[] = { 1, 1, 1, 1, 1, 1, 2, 6, 4, 4 }, outWords[] = { 1, 1, 1, 1, 1, 1, 1, 2, 4, 1 };
    if (fn < RT_MATH_EXP || fn > RT_MATH_LENGTH4 || n < 0 || (n > 0 && (!in || !out))) return fail(RT_E_INVALID, "rt_debug_math: bad argument");
    if (refb && (fn == RT_MATH_ACOS || fn == RT_MATH_ATAN || fn == RT_MATH_ATAN2))
        return fail(RT_E_UNSUPPORTED, "rt_debug_math: RT_BUILTINS_REFERENCE evaluates acos / atan2 only as acospi / atan2pi inside RT_MATH_SPHERE_TEXEL");
    int rc = math_device("rt_debug_math"); if (rc) return rc;
    if (n == 0) return RT_OK;
    const size_t inB = sizeof(uint32_t) * inWords[fn] * (size_t)n, outB = sizeof(uint32_t) * outWords[fn] * (size_t)n;
    uint32_t *dIn = nullptr, *dOut = nullptr;
    hipError_t e = hipMalloc((void**)&dIn, inB);
    if (e == hipSuccess) e = hipMalloc((void**)&dOut, outB);
    if (e == hipSuccess) e = hipMemcpy(dIn, in, inB, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const int grid = (int)std::min<int64_t>((n + kBlock - 1) / kBlock, 65536);
        hipLaunchKernelGGL(refb ? k_debug_math<true> : k_debug_math<false>, dim3(grid), dim3(kBlock), 0, 0, (int)fn, dIn, dOut, (int64_t)n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out, dOut, outB, hipMemcpyDeviceToHost);
    (void)hipFree(dIn); (void)hipFree(dOut);
    if (e != hipSuccess) return fail(RT_E_DEVICE, "rt_debug_math: %s", hipGetErrorString(e));
    return RT_OK;
}
extern "C" int rt_debug_math(int32_t fn, const void* in, void* out, int64_t n) { return rt_debug_math_mode(RT_BUILTINS_DEFAULT, fn, in, out, n); }
extern "C" int rt_debug_math_sweep_mode(int32_t builtins, int32_t fn, int32_t firstBlock, int32_t nBlocks, uint64_t* hashes)
{
    int32_t mode;
    if (!resolve_builtins(builtins, &mode)) return fail(RT_E_INVALID, "rt_debug_math_sweep: builtins = %d is none of RT_BUILTINS_DEFAULT (0), RT_BUILTINS_IEEE (1), RT_BUILTINS_REFERENCE (2)", builtins);
    const bool refb = mode == RT_BUILTINS_REFERENCE;
    constexpr int kBlocks = 1 << (32 - RT_MATH_SWEEP_BLOCK_BITS);
    if (fn < RT_MATH_EXP || fn > RT_MATH_F2I || firstBlock < 0 || nBlocks < 0 || firstBlock + nBlocks > kBlocks || (nBlocks > 0 && !hashes))
        return fail(RT_E_INVALID, "rt_debug_math_sweep: bad argument");
    if (refb && (fn == RT_MATH_ACOS || fn == RT_MATH_ATAN))
        return fail(RT_E_UNSUPPORTED, "rt_debug_math_sweep: RT_BUILTINS_REFERENCE has no acos / atan of its own");
    int rc = math_device("rt_debug_math_sweep"); if (rc) return rc;
    if (nBlocks == 0) return RT_OK;
    unsigned long long* dH = nullptr;
    hipError_t e = hipMalloc((void**)&dH, sizeof(uint64_t) * nBlocks);
    if (e == hipSuccess) e = hipMemset(dH, 0, sizeof(uint64_t) * nBlocks);
    if (e == hipSuccess) {
        const int groups = nBlocks * ((1 << RT_MATH_SWEEP_BLOCK_BITS) / (kBlock * kSweepPerThread));
        hipLaunchKernelGGL(refb ? k_debug_math_sweep<true> : k_debug_math_sweep<false>, dim3(groups), dim3(kBlock), 0, 0, (int)fn, (uint32_t)firstBlock, dH);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(hashes, dH, sizeof(uint64_t) * nBlocks, hipMemcpyDeviceToHost);
    (void)hipFree(dH);
    if (e != hipSuccess) return fail(RT_E_DEVICE, "rt_debug_math_sweep: %s", hipGetErrorString(e));
    return RT_OK;
}
extern "C" int rt_debug_math_sweep(int32_t fn, int32_t firstBlock, int32_t nBlocks, uint64_t* hashes) { return rt_debug_math_sweep_mode(RT_BUILTINS_DEFAULT, fn, firstBlock, nBlocks, hashes); }

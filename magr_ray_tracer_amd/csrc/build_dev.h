// build_dev.h — the driver side of a GPU builder's translation unit (lbvh.hip, sah.hip, sbvh.hip): error reporting, the session a C-ABI
// entry opens on its device, and the tail that rt_build_bvh2 and rt_build_bvh2_sah share around their cores (build_cores.h).
#pragma once
#include <hip/hip_runtime.h>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include "../../include/rt355.h"
#include "build_cores.h"

int rt355_set_error(int code, const char* msg);   // rt355.hip: sets the text rt_last_error() returns

namespace builddev {

using Clock = std::chrono::steady_clock;

inline int build_fail(int code, const char* fmt, ...)   // the message goes to rt_last_error()
{
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    return rt355_set_error(code, buf);
}

inline size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }
inline dim3 grid(uint32_t threads, int block) { return dim3((threads + block - 1) / block); }
inline double ms_since(Clock::time_point t) { return std::chrono::duration<double, std::milli>(Clock::now() - t).count(); }

// Returns from a function that has `who` in scope: out of device memory is RT_E_NOMEM, every other HIP failure RT_E_DEVICE.
#define BUILD_CHK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) \
    return builddev::build_fail(e_ == hipErrorOutOfMemory ? RT_E_NOMEM : RT_E_DEVICE, "%s: %s failed: %s", who, #expr, hipGetErrorString(e_)); } while (0)

// What one C-ABI build call holds on its device once open_session() has succeeded: a stream, the two events around the kernels and up
// to two allocations; released on every exit path.  An owner of more device state derives from it and, in its destructor, calls
// idle() and then drops that state.
struct Session {
    void* mem[2] = { nullptr, nullptr };
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = { nullptr, nullptr };
    int prevDevice = -1;                      // the caller's current device, restored on the way out

    void idle() { if (stream) (void)hipStreamSynchronize(stream); }
    ~Session()
    {
        idle();
        for (void* m : mem) if (m) (void)hipFree(m);
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
        if (prevDevice >= 0) (void)hipSetDevice(prevDevice);
    }
    Session() = default;
    Session(const Session&) = delete;
    Session& operator=(const Session&) = delete;
};

inline int open_session(const char* who, int32_t device, Session& w)
{
    int nDev = 0;
    if (hipGetDeviceCount(&nDev) != hipSuccess || nDev <= 0) return build_fail(RT_E_DEVICE, "%s: no HIP device", who);
    if (device < 0 || device >= nDev) return build_fail(RT_E_INVALID, "%s: device %d out of range (%d devices)", who, device, nDev);
    BUILD_CHK(hipGetDevice(&w.prevDevice));
    BUILD_CHK(hipSetDevice(device));
    BUILD_CHK(hipStreamCreateWithFlags(&w.stream, hipStreamNonBlocking));
    BUILD_CHK(hipEventCreate(&w.ev[0]));
    BUILD_CHK(hipEventCreate(&w.ev[1]));
    return RT_OK;
}

struct FlatTimes { double alloc, built, done; };   // ms since t0: primitives queued for upload, core returned, arrays downloaded

// The wrapper of a core whose tree has at most 2n - 1 nodes and n indices: one allocation (the core's workspace, then the primitives
// and the output arrays), upload of prims[first, first + n), core(work, dPrims, dNodes, dIdx, &built), download, statistics.
template <class Core>
int build_flat(const char* who, Session& w, Clock::time_point t0, int (*work_bytes)(const char*, uint32_t, hipStream_t, size_t*),
               const RtPrimitive* prims, int32_t first, uint32_t n, RtBVHNode2* nodes, int32_t* nNodes, uint32_t* primIdx, RtBuildStats* stats,
               Core core, Built* built = nullptr, FlatTimes* times = nullptr)
{
    const uint32_t cap = 2 * n - 1;
    size_t workBytes = 0;
    if (const int rc = work_bytes(who, n, w.stream, &workBytes)) return rc;
    const size_t oPrim = align_up(workBytes), oNodes = oPrim + align_up(n * sizeof(RtPrimitive)), oIdx = oNodes + align_up((size_t)cap * sizeof(RtBVHNode2));
    const size_t bytes = oIdx + align_up(n * 4ull);
    if (hipMalloc(&w.mem[0], bytes) != hipSuccess) { w.mem[0] = nullptr; return build_fail(RT_E_NOMEM, "%s: %zu bytes of device memory", who, bytes); }
    RtPrimitive* dPrims = (RtPrimitive*)((char*)w.mem[0] + oPrim);
    RtBVHNode2* dNodes = (RtBVHNode2*)((char*)w.mem[0] + oNodes);
    uint32_t* dIdx = (uint32_t*)((char*)w.mem[0] + oIdx);
    BUILD_CHK(hipMemcpyAsync(dPrims, prims + first, n * sizeof(RtPrimitive), hipMemcpyHostToDevice, w.stream));
    FlatTimes t{ ms_since(t0), 0, 0 };

    Built b{};
    if (const int rc = core(w.mem[0], (const RtPrimitive*)dPrims, dNodes, dIdx, &b)) return rc;
    t.built = ms_since(t0);
    BUILD_CHK(hipMemcpyAsync(nodes, dNodes, b.nodes * sizeof(RtBVHNode2), hipMemcpyDeviceToHost, w.stream));
    BUILD_CHK(hipMemcpyAsync(primIdx, dIdx, n * sizeof(uint32_t), hipMemcpyDeviceToHost, w.stream));
    BUILD_CHK(hipStreamSynchronize(w.stream));
    t.done = ms_since(t0);
    *nNodes = (int32_t)b.nodes;
    if (built) *built = b;
    if (times) *times = t;
    if (stats) {
        float ms = 0;
        BUILD_CHK(hipEventElapsedTime(&ms, w.ev[0], w.ev[1]));
        stats->nodes = (int32_t)b.nodes; stats->leaves = (int32_t)b.leaves; stats->depth = (int32_t)b.depth;
        stats->morton_bits = (int32_t)b.mortonBits; stats->sah_cost = b.cost; stats->device_ms = ms;
        stats->wall_ms = std::chrono::duration<float, std::milli>(Clock::now() - t0).count();
        stats->_reserved = 0;
    }
    return RT_OK;
}

} // namespace builddev

// lab: a census of what a CU of this GPU holds at once.  One "holder" workgroup per CU (256 threads, S bytes of LDS, 128 VGPRs: the shape of
// k_shade<.., 256, ..>) stays resident for 20 ms on one stream; 2 ms later a grid of "tenant" workgroups (256 threads, L bytes of LDS, 64
// VGPRs: the shape of k_trace_persist) arrives on another stream, eight per CU, each staying 1 ms.  Every workgroup records the CU it ran on
// (XCC_ID and HW_ID) and its start and end; the host counts, per CU, the most tenants that were resident at one instant inside the
// holder's interval.  Prints the histogram over CUs for each (S, L) on the command line; S = 0: no holder (the tenants alone).
//   hipcc --offload-arch=gfx950 -O2 tools/lab/lds_census.hip -o /tmp/lds_census && /tmp/lds_census 38988:26560 24908:22976
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <thread>
#include <vector>

#define CHK(e) do { hipError_t e_ = (e); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(e_)); return 1; } } while (0)

struct Rec { unsigned long long cu, t0, t1, pad; };
static constexpr long long kTickPerMs = 100000;   // wall_clock64: 100 MHz

__device__ inline unsigned long long cu_key()
{
    const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);     // HW_ID: cu_id [11:8], sh_id [12], se_id [15:13]
    const unsigned xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);   // XCC_ID [3:0]
    return ((unsigned long long)(xcc & 15u) << 8) | ((hw >> 8) & 0xffu);
}
__device__ inline void stay(Rec* rec, long long ticks, unsigned* lds)
{
    const unsigned long long t0 = wall_clock64();
    lds[threadIdx.x] = threadIdx.x;                                    // the allocation is used
    while ((long long)(wall_clock64() - t0) < ticks) __builtin_amdgcn_s_sleep(64);
    if (threadIdx.x == 0) { rec[blockIdx.x].cu = cu_key(); rec[blockIdx.x].t0 = t0; rec[blockIdx.x].t1 = wall_clock64(); rec[blockIdx.x].pad = lds[lds[0] & 255u]; }
}
__global__ __launch_bounds__(256) void holder(Rec* rec, long long ticks)
{
    extern __shared__ unsigned lds[];
    asm volatile("" ::: "v127");
    stay(rec, ticks, lds);
}
__global__ __launch_bounds__(256) void tenant(Rec* rec, long long ticks)
{
    extern __shared__ unsigned lds[];
    asm volatile("" ::: "v63");
    stay(rec, ticks, lds);
}

int main(int argc, char** argv)
{
    hipDeviceProp_t prop;
    CHK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount, perCU = 8;
    hipStream_t sa, sb;
    CHK(hipStreamCreateWithFlags(&sa, hipStreamNonBlocking));
    CHK(hipStreamCreateWithFlags(&sb, hipStreamNonBlocking));
    CHK(hipFuncSetAttribute((const void*)holder, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    CHK(hipFuncSetAttribute((const void*)tenant, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    Rec *dh, *dt;
    CHK(hipMalloc(&dh, sizeof(Rec) * cus));
    CHK(hipMalloc(&dt, sizeof(Rec) * cus * perCU));
    printf("%s: %d CUs, %zu B of LDS per CU\n", prop.gcnArchName, cus, (size_t)prop.maxSharedMemoryPerMultiProcessor);
    for (int a = 1; a < argc; a++) {
        int S = 0, L = 0;
        if (sscanf(argv[a], "%d:%d", &S, &L) != 2 || S < 0 || S > 160 * 1024 || L < 1024 || L > 160 * 1024) { fprintf(stderr, "bad argument %s\n", argv[a]); return 2; }
        CHK(hipMemset(dh, 0, sizeof(Rec) * cus));
        CHK(hipMemset(dt, 0, sizeof(Rec) * cus * perCU));
        CHK(hipDeviceSynchronize());
        if (S > 0) {
            hipLaunchKernelGGL(holder, dim3(cus), dim3(256), S, sa, dh, 20 * kTickPerMs);
            std::this_thread::sleep_for(std::chrono::milliseconds(2));
        }
        hipLaunchKernelGGL(tenant, dim3(cus * perCU), dim3(256), L, sb, dt, 1 * kTickPerMs);
        CHK(hipDeviceSynchronize());
        std::vector<Rec> h(cus), t((size_t)cus * perCU);
        CHK(hipMemcpy(h.data(), dh, sizeof(Rec) * cus, hipMemcpyDeviceToHost));
        CHK(hipMemcpy(t.data(), dt, sizeof(Rec) * cus * perCU, hipMemcpyDeviceToHost));
        std::map<unsigned long long, std::pair<unsigned long long, unsigned long long>> held;   // CU -> the holder's interval
        int doubled = 0;
        for (const Rec& r : h) if (r.t1) { if (held.count(r.cu)) doubled++; held[r.cu] = { r.t0, r.t1 }; }
        std::map<unsigned long long, std::vector<std::pair<unsigned long long, int>>> ev;   // CU -> (time, +1 / -1)
        for (const Rec& r : t) {
            if (!r.t1) continue;
            if (S > 0) { auto it = held.find(r.cu); if (it == held.end() || r.t0 < it->second.first || r.t1 > it->second.second) continue; }
            ev[r.cu].push_back({ r.t0, +1 }); ev[r.cu].push_back({ r.t1, -1 });
        }
        std::map<int, int> hist;
        for (auto& [cu, e] : ev) {
            std::sort(e.begin(), e.end(), [](auto& x, auto& y) { return x.first != y.first ? x.first < y.first : x.second < y.second; });
            int now = 0, most = 0;
            for (auto& x : e) { now += x.second; most = std::max(most, now); }
            hist[most]++;
        }
        printf("holder %6d B, tenants %6d B: CUs seen %zu (holders %zu, two on a CU %d); most tenants resident at once -> CUs:", S, L, ev.size(), held.size(), doubled);
        for (auto& [k, v] : hist) printf("  %d -> %d", k, v);
        printf("\n");
    }
    return 0;
}

// fold_dev.h — the workgroup fold of the SAH and SBVH level kernels (sah.hip, sbvh.hip), device side.  A workgroup's positions meet a
// short run of consecutive nodes: it folds their 64-bit keys (sah_common.h's key_min / key_max) and counters into kSlots LDS slots,
// slot 0 being the lowest node it meets (*sfirst), and then sends only the touched slots to the global arrays.  A kernel
//   init_keys / init_counts / init_first, barrier, atomicMin(sfirst, node), barrier,
//   folds into slot node - *sfirst with lds_min / lds_max / atomicAdd (what it does with a node past the slots is its own), barrier,
//   returns if *sfirst is still kNone, flush_keys / flush_counts to the global arrays at *sfirst * (words per node).
// kBlock is the workgroup size, kWords the slots times the words per node.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sah_common.h"

namespace fold {

__device__ inline void lds_min(uint64_t* p, uint64_t v) { __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ inline void lds_max(uint64_t* p, uint64_t v) { __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ inline void glb_min(uint64_t* p, uint64_t v) { __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void glb_max(uint64_t* p, uint64_t v) { __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <int kBlock, int kWords> __device__ inline void init_keys(uint64_t* smin, uint64_t* smax)
{
    for (int t = threadIdx.x; t < kWords; t += kBlock) { smin[t] = sah::kKeyMinEmpty; smax[t] = sah::kKeyMaxEmpty; }
}
template <int kBlock, int kWords> __device__ inline void init_counts(uint32_t* scnt)
{
    for (int t = threadIdx.x; t < kWords; t += kBlock) scnt[t] = 0;
}
__device__ inline void init_first(uint32_t* sfirst) { if (threadIdx.x == 0) *sfirst = sah::kNone; }

// touched slots only: their nodes exist, so gmin / gmax (the global keys of node *sfirst) are written inside the level's arrays
template <int kBlock, int kWords> __device__ inline void flush_keys(const uint64_t* smin, const uint64_t* smax, uint64_t* gmin, uint64_t* gmax)
{
    for (int t = threadIdx.x; t < kWords; t += kBlock) {
        if (smin[t] != sah::kKeyMinEmpty) glb_min(&gmin[t], smin[t]);
        if (smax[t] != sah::kKeyMaxEmpty) glb_max(&gmax[t], smax[t]);
    }
}
template <int kBlock, int kWords> __device__ inline void flush_counts(const uint32_t* scnt, uint32_t* gcnt)
{
    for (int t = threadIdx.x; t < kWords; t += kBlock)
        if (scnt[t]) atomicAdd(&gcnt[t], scnt[t]);
}

} // namespace fold

// g2048_per_max.h -- the priority a push into the prioritized replay ring gives its entries (g2048_per.h has the rule): the
// maximum of the live priorities, by a memset and one small launch in front of whatever writes the entries. Device and host code
// of the library's .hip files: g2048_per.hip (g2048_per_push) and g2048_qnet_collect.hip (g2048_qnet_collect) enqueue exactly this.
#pragma once
#include <hip/hip_runtime.h>

#include "g2048_host.h"
#include "g2048_per.h"

namespace {

using namespace g2048;

constexpr int kPerBlock = 256;                        // threads of the kernels that walk the buffer

// *max_bits (zeroed before the launch) <- the bits of the largest live priority; priorities are positive, so their bits order
// as they do
__global__ __launch_bounds__(kPerBlock) void per_max_kernel(const float *__restrict__ priorities, size_t capacity, size_t size, size_t head,
                                                           uint32_t *max_bits)
{
    uint32_t m = 0u;
    for (size_t i = (size_t)blockIdx.x * kPerBlock + threadIdx.x; i < size; i += (size_t)gridDim.x * kPerBlock)
        m = max(m, __float_as_uint(priorities[per_slot(head, i, capacity)]));
    for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off));
    if ((threadIdx.x & 63u) == 0u && m != 0u) atomicMax(max_bits, m);
}

// the two stream operations in front of a push into a ring that holds entries (size > 0); `what`: "<entry point>: hipMemsetAsync"
inline int per_max_enqueue(const char *what, const float *priorities, size_t capacity, size_t size, size_t head, uint32_t *max_bits, hipStream_t s)
{
    const int rc = check_hip(hipMemsetAsync(max_bits, 0, sizeof(uint32_t), s), what);
    if (rc != G2048_OK) return rc;
    const unsigned blocks = blocks_for(size, kPerBlock);
    hipLaunchKernelGGL(per_max_kernel, dim3(blocks < 256u ? blocks : 256u), dim3(kPerBlock), 0, s, priorities, capacity, size, head, max_bits);
    return G2048_OK;
}

}  // namespace
